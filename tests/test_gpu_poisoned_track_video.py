"""The track-video entries (vgg_track_owner / vgg_track_resolve) on poisoned, guard-banded memory, in the form of
tests/test_gpu_poisoned_video_output.py: the parity cases of tests/test_gpu_track_video.py run with every ``empty``-family
buffer (the owner grid and the output video among them) filled with 0x00, 0xFF and 0x7F and framed by guard bands; what
they read back must be run-to-run deterministic, bit-identical across the patterns, and no guard byte may change."""
import pytest

from tests import test_gpu_track_video as TTV
from tests.test_gpu_poisoned_memory import _check_poisoned

pytestmark = pytest.mark.gpu

CASES = {
    # the runner's call; frames before query_frame, an odd canvas width (scalar stores), mode "cool"
    "default": lambda mp: TTV.test_render_equals_reference("default"),
    "cool_lw2_pad3": lambda mp: TTV.test_render_equals_reference("cool_lw2_pad3"),
    # the padded, dword-store path with one frame per owner grid (the grid is cleared and reused chunk after chunk)
    "pad4_one_frame_chunks": lambda mp: TTV.test_one_frame_per_chunk_gives_the_same_bits("pad4"),
    # most pixels contested, frames streamed from host memory two at a time
    "contested_host": lambda mp: TTV.test_frames_streamed_from_host_memory("contested", 2),
    "lw3_uint8": lambda mp: TTV.test_uint8_frames_give_the_same_bits("lw3_novis"),
    "one_frame": lambda mp: TTV.test_visualizer_equals_reference("one_frame"),
}


@pytest.mark.parametrize("name", list(CASES))
def test_track_video_entries_on_poisoned_memory(name):
    _check_poisoned(CASES[name])
