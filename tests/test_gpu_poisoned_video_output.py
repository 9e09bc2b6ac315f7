"""The point-colour entries (vgg_color_gather / vgg_color_reduce) on poisoned, guard-banded memory, in the form of
tests/test_gpu_poisoned_memory.py: the parity cases of tests/test_gpu_video_output.py run with every ``empty``-family
buffer filled with 0x00, 0xFF and 0x7F and framed by guard bands; what they read back must be run-to-run deterministic,
bit-identical across the patterns and never the pattern, and no guard byte may change."""
import pytest

from tests import test_gpu_video_output as TV
from tests.test_gpu_poisoned_memory import _check_poisoned

pytestmark = pytest.mark.gpu

CASES = {
    # non-square frames with every edge of the index rule (a colourless point among them), then the output
    "nonsquare_radial": lambda mp: (TV.test_colors_match_reference("nonsquare_radial"),
                                    TV.test_dicts_to_output_matches_reference("nonsquare_radial")),
    # reverse on square frames, in chunks of frames held in host memory
    "square_reverse_host_chunks": lambda mp: TV.check_colors(
        *TV.gpu_geometry(TV.load("square_reverse")).update_points_color(
            TV.frames_of(TV.load("square_reverse")).cpu(), reverse=True, frame_chunk=4), TV.load("square_reverse")),
    # the error path: the status word is read back
    "below_w_raises": lambda mp: TV.test_index_out_of_range_raises("below_w_raises"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_color_entries_on_poisoned_memory(name):
    _check_poisoned(CASES[name])
