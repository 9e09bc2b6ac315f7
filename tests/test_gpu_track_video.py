"""The track video on the MI355X against the reference's own output (tests/golden/track_video_<case>.npz, written by
scripts/make_golden_track_video.py from the reference's ``Visualizer.visualize`` with the real PIL): every comparison is
``torch.equal`` on uint8 frames.  Reads nothing but tests/golden/."""
import numpy as np
import pytest
import torch

from tests.test_track_video_host import CASES, load
from vggsfm_amd import track_video as TV
from vggsfm_amd.runners import GeometryRunner
from vggsfm_amd.utils.visualizer import Visualizer

pytestmark = pytest.mark.gpu


def D(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def inputs(g, uint8=False, host=False):
    """(video (1,T,3,H,W), tracks (1,T,N,2), visibility (1,T,N,1) or None): float frames carry the golden's fraction."""
    frames = torch.from_numpy(g["frames"]) if uint8 else torch.from_numpy(g["frames"].astype(np.float32) + g["frame_frac"])
    video = frames[None] if host else frames[None].cuda()
    vis = None if g["visibility"] is None else D(g["visibility"])[None, :, :, None]
    return video, D(g["tracks"])[None], vis


def check(out, g):
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (1,) + g["expect"].shape
    want = torch.from_numpy(g["expect"])[None]
    got = out.cpu()
    assert torch.equal(got, want), f"{int((got != want).sum())} bytes differ"


@pytest.mark.parametrize("case", CASES)
def test_render_equals_reference(case):
    g = load(case)
    check(TV.render(*inputs(g), **g["options"]), g)


@pytest.mark.parametrize("case", CASES)
def test_visualizer_equals_reference(case):
    g = load(case)
    o = g["options"]
    viz = Visualizer(mode=o["mode"], linewidth=o["linewidth"], pad_value=o["pad_value"], show_first_frame=o["show_first_frame"])
    check(viz.visualize(*inputs(g), query_frame=o["query_frame"], save_video=False), g)


@pytest.mark.parametrize("case", CASES)
def test_one_frame_per_chunk_gives_the_same_bits(case):
    g = load(case)
    check(TV.render(*inputs(g), max_grid_cells=1, **g["options"]), g)


@pytest.mark.parametrize("case", CASES)
def test_uint8_frames_give_the_same_bits(case):
    g = load(case)
    check(TV.render(*inputs(g, uint8=True), **g["options"]), g)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("frame_chunk", [None, 2])
def test_frames_streamed_from_host_memory(case, frame_chunk):
    g = load(case)
    video, tracks, vis = inputs(g, host=True)
    assert not video.is_cuda
    check(TV.render(video, tracks, vis, frame_chunk=frame_chunk, **g["options"]), g)


@pytest.mark.parametrize("case", ["default", "contested"])
def test_two_runs_give_the_same_bits(case):
    g = load(case)
    a = TV.render(*inputs(g), **g["options"])
    b = TV.render(*inputs(g), **g["options"])
    assert torch.equal(a, b)


def test_float64_tracks_and_visibility():
    """The same values in float64 truncate alike (float32 -> float64 is exact, and so is the pad addition here)."""
    g = load("pad4")
    video, tracks, vis = inputs(g)
    check(TV.render(video, tracks.double(), vis.double(), **g["options"]), g)


def test_draw_tracks_on_video_takes_padded_input():
    """draw_tracks_on_video is visualize without the padding step."""
    g = load("lw3_novis")
    o = g["options"]
    assert o["pad_value"] == 0
    video, tracks, vis = inputs(g)
    viz = Visualizer(mode=o["mode"], linewidth=o["linewidth"], show_first_frame=o["show_first_frame"])
    check(viz.draw_tracks_on_video(video, tracks, vis, query_frame=o["query_frame"]), g)


def test_geometry_runner_visualize_tracks():
    """runner.py:445-450: images in [0, 1] times 255, pred_vis (1,S,N) scores, linewidth 1."""
    g = load("default")
    images = (torch.from_numpy(g["frames"].astype(np.float32)) + float(g["frame_frac"])).cuda()[None] / 255
    # (x / 255 * 255 need not return x; the fraction keeps the product well inside its integer's interval)
    assert torch.equal((images * 255).to(torch.uint8).cpu()[0], torch.from_numpy(g["frames"]))
    out = GeometryRunner().visualize_tracks(images, D(g["tracks"])[None], D(g["visibility"])[None])
    check(out, g)


def test_frame_values_outside_the_byte_range_saturate():
    video = torch.tensor([-3.5, 0.0, 255.9, 256.0, 1e9, float("nan"), 17.99, float("inf")], device="cuda")
    video = video.reshape(1, 1, 1, 1, 8).expand(1, 1, 3, 2, 8).contiguous()
    tracks = torch.full((1, 1, 1, 2), -50.0, device="cuda")
    out = TV.render(video, tracks, show_first_frame=0)
    assert out[0, 0, 1, 1].tolist() == [0, 0, 255, 255, 255, 0, 17, 255]
