"""The registration entries on poisoned, guard-banded memory: cases of tests/test_gpu_icp.py through the checks of
tests/test_gpu_poisoned_memory.py (bit-identical read-backs across 0x00 / 0xFF / 0x7F, no guard byte changed, the cases' own
assertions under every pattern).  The workspace, the sums, the pairs and the normals are allocated by torch.empty, so only
what the entries wrote may come back: M = 255 and 257 are no multiple of the 256 lanes of a workgroup, most of the 512
workgroups have no query at all and must still write their row of zeros, M = 0 and N = 0 are launched and write zeros, and
with out_index off (the whole loop) nothing but the state, the history and the sums is touched."""
import pytest

from tests import test_gpu_icp as TI
from tests.test_gpu_poisoned_memory import _check_poisoned

pytestmark = pytest.mark.gpu

CASES = {
    "m255_m257": lambda mp: (TI.test_step_matches_restatement("m255"), TI.test_step_matches_restatement("m257"),
                             TI.test_step_matches_restatement("mesh_f0")),
    "no_ops": lambda mp: (TI.test_step_matches_restatement("m0"), TI.test_step_matches_restatement("n0"),
                          TI.test_step_matches_restatement("none_within")),
    "index_off": lambda mp: (TI.test_trajectory_follows_the_restatement_and_recovers_the_truth("plane_scale"),
                             TI.test_update_solves_the_read_back_system("mesh_plane_metric0")),
    "normals": lambda mp: (TI.test_radius_normals_match_restatement("nonfinite"), TI.test_radius_normals_match_restatement("lonely"),
                           TI.test_step_matches_restatement("nonfinite")),
}


@pytest.mark.parametrize("name", list(CASES))
def test_icp_entry_on_poisoned_memory(name):
    _check_poisoned(CASES[name])
