"""The track video's formulation and host side, without a device (vggsfm_amd/track_video.py).

The goldens tests/golden/track_video_<case>.npz are the reference's own ``Visualizer.visualize`` output
(scripts/make_golden_track_video.py).  Here the rule the kernels implement -- two stencils per radius, each pixel to the
highest track index that covers it, colours from matplotlib's tables -- is restated in numpy and must reproduce every
golden bit for bit; the stencil tables must be Pillow's; every unsupported option must be refused before the device is
touched.  There is no tolerance: every comparison is equality of uint8 frames."""
import glob
import inspect
import os

import numpy as np
import pytest
import torch

from oracle import ref_harness
from vggsfm_amd import _lib
from vggsfm_amd import track_video as TV
from vggsfm_amd.runners import GeometryConfig, GeometryRunner
from vggsfm_amd.utils.visualizer import Visualizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = sorted(os.path.basename(p)[len("track_video_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "track_video_*.npz")))


def load(case):
    g = np.load(os.path.join(GOLDEN, f"track_video_{case}.npz"), allow_pickle=False)
    return dict(frames=g["frames"], frame_frac=np.float32(g["frame_frac"]), tracks=g["tracks"],
                visibility=g["visibility"] if "visibility" in g.files else None, expect=g["expect"],
                options=dict(mode=str(g["mode"]), linewidth=int(g["linewidth"]), pad_value=int(g["pad_value"]),
                             query_frame=int(g["query_frame"]), show_first_frame=int(g["show_first_frame"])))


def test_the_cases_are_all_there():
    assert CASES == sorted(["default", "cool_lw2_pad3", "lw3_novis", "pad4", "contested", "single_track", "one_frame"])


def test_the_cases_cover_what_they_claim():
    g = {c: load(c) for c in CASES}
    d = g["default"]
    assert d["options"] == dict(mode="rainbow", linewidth=1, pad_value=0, query_frame=0, show_first_frame=3)
    v = d["visibility"]
    assert (v == 0).any() and np.isnan(v).any() and np.signbit(v[v == 0]).any()
    H, W = d["frames"].shape[-2:]
    x, y = d["tracks"][..., 0], d["tracks"][..., 1]
    assert (x < -2).any() and (x > W + 2).any() and (y < -2).any() and (y > H + 2).any()       # off every side
    for val in (0.4, -0.6, -1.2, 1.0):                                                      # truncation to 0 or not
        assert (d["tracks"] == np.float32(val)).any()
    c = g["cool_lw2_pad3"]
    assert c["options"]["mode"] == "cool" and c["options"]["linewidth"] == 2 and c["options"]["pad_value"] % 2 == 1
    assert c["options"]["query_frame"] > 0 and c["options"]["show_first_frame"] == 0 and c["visibility"].dtype == bool
    assert (c["frames"].shape[-1] + 2 * c["options"]["pad_value"]) % 4 != 0
    assert g["lw3_novis"]["options"]["linewidth"] == 3 and g["lw3_novis"]["visibility"] is None
    assert g["lw3_novis"]["frames"].shape[-1] % 4 != 0
    k = g["contested"]
    assert k["tracks"].shape[1] > k["frames"].shape[-1] * k["frames"].shape[-2]
    assert g["single_track"]["tracks"].shape[1] == 1 and g["one_frame"]["frames"].shape[0] == 1


@pytest.mark.parametrize("case", CASES)
def test_numpy_restatement_equals_the_reference(case):
    g = load(case)
    out = TV.render_numpy(g["frames"], g["tracks"], g["visibility"], **g["options"])
    assert out.dtype == np.uint8 and out.shape == g["expect"].shape
    assert np.array_equal(out, g["expect"]), f"{(out != g['expect']).sum()} bytes differ"


def test_single_track_is_drawn():
    g = load("single_track")
    first = g["options"]["show_first_frame"] - 1
    changed = (g["expect"][first:] != g["frames"]).any(1).reshape(len(g["frames"]), -1).sum(1).tolist()
    H, W = g["frames"].shape[-2:]
    x, y, v = g["tracks"][:, 0, 0], g["tracks"][:, 0, 1], g["visibility"][:, 0]
    inside = (x > 3) & (x < W - 3) & (y > 3) & (y < H - 3)
    # (the frame's own pixels differ from the one colour everywhere: a whole stencil changes, 21 filled or 12 outline)
    assert changed == [0 if not i else (12 if s == 0 else 21) for i, s in zip(inside, v)] and sorted(changed) == [0, 12, 21]


def test_stencil_tables_are_well_formed():
    assert len(TV.FILLED_ROWS) == len(TV.OUTLINE_ROWS) == TV.MAX_RADIUS + 1
    for r in range(TV.MAX_RADIUS + 1):
        for rows in (TV.FILLED_ROWS[r], TV.OUTLINE_ROWS[r]):
            assert len(rows) == 2 * r + 1 and all(0 <= m < 1 << (2 * r + 1) for m in rows)
        f, o = TV.stencil(r, True), TV.stencil(r, False)
        assert np.array_equal(f, f.T) and np.array_equal(f, f[::-1]) and np.array_equal(o, o.T) and np.array_equal(o, o[::-1])
        if r > 0:
            assert not (o & ~f).any()
    assert TV.stencil(2, True).sum() == 21 and TV.stencil(2, False).sum() == 12
    corners = np.ones((5, 5), bool)
    corners[[0, 0, 4, 4], [0, 4, 0, 4]] = False
    assert np.array_equal(TV.stencil(2, True), corners)


@pytest.mark.parametrize("filled", [True, False])
def test_stencil_tables_equal_pillow(filled):
    Image = pytest.importorskip("PIL.Image")
    ImageDraw = pytest.importorskip("PIL.ImageDraw")
    for r in range(TV.MAX_RADIUS + 1):
        for cx, cy in ((40, 40), (17, 52), (3, 5), (60, 1)):            # translated, and clipped at the borders
            im = Image.new("RGB", (64, 64))
            ImageDraw.Draw(im).ellipse([(cx - r, cy - r), (cx + r, cy + r)], fill=(9, 8, 7) if filled else None, outline=(9, 8, 7))
            got = np.array(im)[..., 0] > 0
            want = np.zeros((64 + 2 * r, 64 + 2 * r), bool)
            want[cy:cy + 2 * r + 1, cx:cx + 2 * r + 1] = TV.stencil(r, filled)
            assert np.array_equal(got, want[r:r + 64, r:r + 64]), (r, cx, cy)


@pytest.mark.skipif(not ref_harness.available(), reason="the reference tree is not here")
@pytest.mark.parametrize("case", ["default", "cool_lw2_pad3"])
def test_goldens_equal_the_live_reference(case):
    pytest.importorskip("PIL.Image")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden_track_video", os.path.join(ROOT, "scripts", "make_golden_track_video.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    frames, tracks, vis = M.make_inputs(M.CASES[case])
    g = load(case)
    assert np.array_equal(frames, g["frames"]) and np.array_equal(tracks, g["tracks"])
    assert np.array_equal(M.run_reference(M.reference_visualizer(), M.CASES[case], frames, tracks, vis), g["expect"])


def test_colour_tables():
    one = TV.rainbow_colors([7])
    assert one.tolist() == TV.rainbow_colors([7, 7, 7])[:1].tolist()                  # y_min == y_max: index 0
    lut, n = TV.pack_lut(TV.colormap_lut("gist_rainbow"))
    assert one[0] == lut[0] and TV.rainbow_colors([0, 10])[1] == lut[n - 1]
    cool, _ = TV.pack_lut(TV.colormap_lut("cool"))
    assert TV.cool_colors(4).tolist() == [cool[0], cool[64], cool[128], cool[192]]


# --- refusals: before anything is launched (no library is loaded, no device touched) -------------------------------------
def _inputs(T=3, N=5, H=8, W=12):
    return torch.zeros(1, T, 3, H, W), torch.ones(1, T, N, 2) * 4, torch.ones(1, T, N, 1)


@pytest.fixture
def no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device library was reached")
    monkeypatch.setattr(_lib, "lib", boom)


@pytest.mark.parametrize("init, call, word", [
    (dict(mode="optical_flow"), {}, "optical_flow"),
    (dict(grayscale=True), {}, "grayscale"),
    (dict(tracks_leave_trace=2), {}, "tracks_leave_trace"),
    (dict(tracks_leave_trace=-1), {}, "tracks_leave_trace"),
    ({}, dict(segm_mask=torch.zeros(1, 1, 8, 12)), "segm_mask"),
    ({}, dict(gt_tracks=torch.zeros(1, 3, 5, 2)), "gt_tracks"),
    ({}, dict(compensate_for_camera_motion=True), "compensate_for_camera_motion"),
])
def test_unsupported_options_raise_not_implemented(no_device, init, call, word):
    video, tracks, vis = _inputs()
    with pytest.raises(NotImplementedError, match=word):
        Visualizer(**init).visualize(video, tracks, vis, save_video=False, **call)
    if call:
        with pytest.raises(NotImplementedError, match=word):
            Visualizer().draw_tracks_on_video(video, tracks, vis, **call)


def test_value_errors(no_device):
    video, tracks, vis = _inputs()
    bad = [
        (dict(video=video.expand(2, -1, -1, -1, -1), tracks=tracks), {}, "batch size"),
        (dict(video=video[:, :, :2], tracks=tracks), {}, "channels"),
        (dict(video=video, tracks=tracks), dict(query_frame=3), "query_frame"),
        (dict(video=video, tracks=tracks), dict(query_frame=-1), "query_frame"),
        (dict(video=video, tracks=tracks), dict(mode="viridis"), "unknown mode"),
        (dict(video=video, tracks=tracks), dict(linewidth=8), "linewidth"),
        (dict(video=video, tracks=tracks[:, :2]), {}, "tracks"),
        (dict(video=video, tracks=tracks, visibility=vis[:, :, :3]), {}, "visibility"),
        (dict(video=video.double(), tracks=tracks), {}, "video"),
    ]
    for k, nonfinite in enumerate((float("nan"), float("inf"), -float("inf"))):
        t = tracks.clone()
        t[0, 2, k, 1] = nonfinite
        bad.append((dict(video=video, tracks=t), {}, "non-finite"))
    for args, kw, word in bad:
        with pytest.raises(ValueError, match=word):
            TV.render(**args, **kw)
    with pytest.raises(ValueError, match="unknown mode"):
        Visualizer(mode="viridis")
    with pytest.raises(ValueError, match="linewidth"):
        Visualizer(linewidth=8)
    assert TV.radius_of(7.5) == 15 and TV.radius_of(0.5) == 1


def test_save_video_without_imageio_says_so(tmp_path, monkeypatch):
    import builtins
    real = builtins.__import__

    def fake(name, *a, **k):
        if name == "imageio":
            raise ImportError("No module named 'imageio'")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", fake)
    with pytest.raises(ImportError, match="imageio"):
        Visualizer(save_dir=str(tmp_path)).save_video(torch.zeros(1, 5, 3, 4, 4, dtype=torch.uint8), "track")


def test_save_video_keeps_the_reference_selection(tmp_path, monkeypatch):
    """frames[2:-1] to save_dir/<filename>.mp4 at fps, or the whole tensor to a tensorboard writer."""
    import sys
    import types
    written = {}

    class Writer:
        def __init__(self, path, fps):
            written.update(path=path, fps=fps, frames=[])

        def append_data(self, frame):
            written["frames"].append(frame)

        def close(self):
            written["closed"] = True
    monkeypatch.setitem(sys.modules, "imageio", types.SimpleNamespace(get_writer=lambda path, fps: Writer(path, fps)))
    video = torch.arange(6, dtype=torch.uint8).reshape(1, 6, 1, 1, 1).expand(1, 6, 3, 4, 5).contiguous()
    Visualizer(save_dir=str(tmp_path / "visuals"), fps=7).save_video(video, "track")
    assert written["path"] == str(tmp_path / "visuals" / "track.mp4") and written["fps"] == 7 and written["closed"]
    assert [int(f[0, 0, 0]) for f in written["frames"]] == [2, 3, 4] and written["frames"][0].shape == (4, 5, 3)
    calls = []
    tb = types.SimpleNamespace(add_video=lambda name, v, global_step, fps: calls.append((name, tuple(v.shape), global_step, fps)))
    Visualizer(fps=2).save_video(video, "track", writer=tb, step=9)
    assert calls == [("track", (1, 6, 3, 4, 5), 9, 2)]


def test_interfaces():
    assert GeometryConfig().visual_tracks is False
    assert list(inspect.signature(GeometryRunner.visualize_tracks).parameters) == ["self", "images", "pred_track", "pred_vis",
                                                                                    "output_dir"]
    p = inspect.signature(TV.render).parameters
    assert list(p)[:3] == ["video", "tracks", "visibility"]
    for name, default in (("mode", "rainbow"), ("linewidth", 1), ("pad_value", 0), ("query_frame", 0), ("show_first_frame", 3),
                          ("max_grid_cells", TV.MAX_GRID_CELLS), ("frame_chunk", None)):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default == default
    assert {"vgg_track_owner", "vgg_track_resolve"} <= set(_lib.EXPORTED)
