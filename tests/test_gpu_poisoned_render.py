"""The rasteriser's entries on poisoned, guard-banded memory: cases of tests/test_gpu_render.py through the checks of
tests/test_gpu_poisoned_memory.py (bit-identical read-backs across 0x00 / 0xFF / 0x7F, no guard byte changed, the cases' own
assertions under every pattern).  The maps are allocated by torch.empty, so only what the entries wrote may come back: the
21 x 35 frames (735 pixels) are no multiple of the 256 lanes of a workgroup (the guarded stores of the resolve matter, and a
box clamped to the frame must stay inside it), the empty render writes 'none' to every pixel, absent attributes leave their
outputs alone, and the skippable faces load nothing at their bad rows.  The key buffer is the one buffer whose initial
contents are an input: every case fills it itself (render.new_keys)."""
import pytest

from tests import test_gpu_render as TR
from tests.test_gpu_poisoned_memory import _check_poisoned

pytestmark = pytest.mark.gpu

CASES = {
    "frames_21x35": lambda mp: (TR.test_render_matches_restatement("plane_21x35"), TR.test_render_matches_restatement("sphere_21x35"),
                                TR.test_render_matches_restatement("fill_21x35")),
    "empty_render": lambda mp: (TR.test_render_matches_restatement("no_face"), TR.test_render_matches_restatement("one_face")),
    "outputs_off": lambda mp: TR.test_outputs_off_touch_nothing_else(),
    "skippable_faces": lambda mp: (TR.test_render_matches_restatement("skippable"),
                                   TR.test_render_matches_restatement("skippable_21x35"),
                                   TR.test_visible_points_match_restatement()),
}


@pytest.mark.parametrize("name", list(CASES))
def test_render_entry_on_poisoned_memory(name):
    _check_poisoned(CASES[name])
