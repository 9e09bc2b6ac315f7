"""The tracker's entries on poisoned, guard-banded memory: three cases of tests/test_gpu_klt.py through the checks of
tests/test_gpu_poisoned_memory.py (bit-identical read-backs across 0x00 / 0xFF / 0x7F, no guard byte changed, the cases'
own assertions under every pattern)."""
import pytest

from tests import test_gpu_klt as TK
from tests.test_gpu_poisoned_memory import _check_poisoned

pytestmark = pytest.mark.gpu

CASES = {
    "pyramid_33x47": lambda mp: TK.test_pyramid_bit_exact((33, 47)),
    "selection_plateau": lambda mp: (TK.test_selection_on_a_plateau_of_the_response(),
                                     TK.test_selection_matches_restatement_on_the_kernels_response("plateau_image")),
    "lk_n5": lambda mp: (TK.test_lk_matches_restatement("n5_r7_l3", "fixed10"), TK.test_lk_matches_restatement("n5_r4_l1", "eps")),
}


@pytest.mark.parametrize("name", list(CASES))
def test_klt_entry_on_poisoned_memory(name):
    _check_poisoned(CASES[name])
