"""The multi-view stereo entries on poisoned, guard-banded memory: cases of tests/test_gpu_mvs.py through the checks of
tests/test_gpu_poisoned_memory.py (bit-identical read-backs across 0x00 / 0xFF / 0x7F, no guard byte changed, the cases'
own assertions under every pattern).  The frame that is no multiple of the 16 x 16 tile is the one whose guarded stores
matter; without a cost volume the three maps are the only outputs."""
import pytest

from tests import test_gpu_mvs as TM
from tests.test_gpu_poisoned_memory import _check_poisoned

pytestmark = pytest.mark.gpu

CASES = {
    "sweep_21x35": lambda mp: TM.test_sweep_matches_restatement("k08_21x35"),
    "sweep_r1_r3_M8": lambda mp: (TM.test_sweep_matches_restatement("r1"), TM.test_sweep_matches_restatement("r3"),
                                  TM.test_sweep_matches_restatement("M8")),
    "sweep_invalid_everywhere": lambda mp: (TM.test_sweep_matches_restatement("facing_away"),
                                            TM.test_sweep_matches_restatement("constant_reference")),
    "sweep_without_cost": lambda mp: TM.test_sweep_without_cost_volume_gives_the_same_bits("k08_21x35"),
    "filter": lambda mp: (TM.test_filter_matches_restatement("holes_mc2"), TM.test_filter_matches_restatement("two_ray_maps"),
                          TM.test_filter_matches_restatement("disagree_mc1")),
}


@pytest.mark.parametrize("name", list(CASES))
def test_mvs_entry_on_poisoned_memory(name):
    _check_poisoned(CASES[name])
