"""The fusion entries on poisoned, guard-banded memory: cases of tests/test_gpu_fusion.py through the checks of
tests/test_gpu_poisoned_memory.py (bit-identical read-backs across 0x00 / 0xFF / 0x7F, no guard byte changed, the cases'
own assertions under every pattern).  The outputs, the staged points and the workgroups' counts are allocated by
torch.empty, so only what the entries wrote may come back: the 21 x 35 frame is no multiple of the 16 x 16 tile nor of the
256 pixels of a workgroup (its guarded stores matter), the cloud of 0 points returns nothing of the one row it allocates,
and the `claimed` map is read back whole."""
import pytest

from tests import test_gpu_fusion as TF
from tests.test_gpu_poisoned_memory import _check_poisoned

pytestmark = pytest.mark.gpu

CASES = {
    "normals_21x35_holes": lambda mp: (TF.test_normals_match_restatement("k08_21x35"), TF.test_normals_match_restatement("holes")),
    "fusion_21x35": lambda mp: TF.test_fusion_matches_restatement("k08_21x35"),
    "fusion_no_points": lambda mp: (TF.test_fusion_matches_restatement("all_zero"), TF.test_fusion_matches_restatement("off_mv2")),
    "fusion_outputs_off_and_auto": lambda mp: (TF.test_fusion_matches_restatement("no_normals"),
                                               TF.test_fusion_matches_restatement("no_colors"),
                                               TF.test_python_surface_and_defaults()),
}


@pytest.mark.parametrize("name", list(CASES))
def test_fusion_entry_on_poisoned_memory(name):
    _check_poisoned(CASES[name])
