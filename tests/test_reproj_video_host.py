"""Host-side checks of the reprojection video (vggsfm_amd/reproj_video.py): the raster rule's geometry (restated in numpy),
the recorded draw lists against an independent restatement of the reference's visibility rule and colours, colormap
tables, chunking, validation, the OpenCV requirement of the video writer, and the C-ABI entries."""
import math
import os
import re
import sys

import numpy as np
import pytest

from vggsfm_amd import _lib
from vggsfm_amd import reproj_video as RV
from vggsfm_amd.utils.utils import save_video_with_reprojections

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CASES = ["center_r3", "origin_r1", "order_r5", "center_r0", "single_point"]


def coverage(a, b, r):
    """Raster rule: the number of the 4 x 4 sub-samples (offsets (2i - 3) / 8) of pixel (x, y) inside the disc of radius r
    around (cx, cy), a = x - cx, b = y - cy; r = 0 covers the centre pixel fully."""
    a, b = np.asarray(a), np.asarray(b)
    if r == 0:
        return np.where((a == 0) & (b == 0), 16, 0)
    k = np.zeros(np.broadcast(a, b).shape, np.int64)
    for i in range(4):
        for j in range(4):
            k += ((8 * a + 2 * i - 3) ** 2 + (8 * b + 2 * j - 3) ** 2 <= 64 * r * r)
    return k


@pytest.mark.parametrize("r", [1, 2, 3, 5, 8, 32])
def test_raster_rule_geometry(r):
    span = r + 3
    b, a = np.mgrid[-span:span + 1, -span:span + 1]
    k = coverage(a, b, r)
    dist = np.hypot(a, b)
    half = 3 * math.sqrt(2) / 8                     # the farthest sub-sample from the pixel centre
    assert (k[dist <= r - half] == 16).all()
    assert (k[dist > r + half] == 0).all()
    assert (k[(np.abs(a) > r) | (np.abs(b) > r)] == 0).all()      # a margin of r around the image is enough
    assert k[span, span] == 16 and ((k >= 0) & (k <= 16)).all()
    for t in (lambda m: m[::-1], lambda m: m[:, ::-1], lambda m: m.T, lambda m: m[::-1, ::-1], lambda m: m.T[::-1],
              lambda m: m.T[:, ::-1], lambda m: m.T[::-1, ::-1]):
        assert np.array_equal(t(k), k)              # the eight symmetries of the grid


def test_raster_rule_radius_zero():
    b, a = np.mgrid[-2:3, -2:3]
    k = coverage(a, b, 0)
    assert k[2, 2] == 16 and k.sum() == 16


def _golden(case):
    return np.load(os.path.join(GOLD, f"reproj_video_{case}.npz"), allow_pickle=False)


def _visible_by_sort(uvs_int, depths):
    """Step 4 restated without the reference's loop: per pixel, the first row of the (depth key, row) order wins, where
    the key orders NaN first and does not distinguish -0.0 from +0.0."""
    n = len(depths)
    d = np.where(depths == 0, 0.0, depths)
    isnan = np.isnan(d)
    order = np.lexsort((np.arange(n), np.where(isnan, 0.0, d), ~isnan, uvs_int[:, 1], uvs_int[:, 0]))
    u = uvs_int[order]
    first = np.ones(n, bool)
    first[1:] = (u[1:] != u[:-1]).any(axis=1)
    mask = np.zeros(n, bool)
    mask[order[first]] = True
    return mask


def _colours(g, xyzid):
    """Steps 1-2 from the recorded statistics and colormap table (matplotlib's Colormap.__call__ restated)."""
    st, mode, lut = g["stats"], str(g["mode"]), g["lut"]
    N = len(lut) - 3
    with np.errstate(all="ignore"):
        if mode == "point_order":
            x = xyzid[:, 3] / st[5]
        else:
            dis = np.linalg.norm(xyzid[:, :3] - (st[:3] if mode == "dis_to_center" else 0.0), axis=1)
            x = (dis - st[3]) / (st[4] - st[3])
        xa = x * N
        xa[xa == N] = N - 1
        idx = np.where(np.isnan(xa), N + 2, np.where(xa < 0, N, np.where(xa >= N, N + 1, 0)))
        inner = ~np.isnan(xa) & (xa >= 0) & (xa < N)
        idx[inner] = xa[inner].astype(int)
    return (lut[idx, :3] * 255).astype(int)


@pytest.mark.parametrize("case", CASES)
def test_golden_draw_lists_follow_the_visibility_rule(case):
    g = _golden(case)
    keys = [str(k) for k in g["keys"]]
    for j, n in enumerate(str(d) for d in g["drawn"]):
        uvd, xyzid = g[f"uvd_{keys.index(n)}"], g[f"xyzid_{keys.index(n)}"]
        uvs_int = np.round(uvd[:, :2]).astype(int)
        mask = _visible_by_sort(uvs_int, uvd[:, 2])
        circles = g[f"circles_{j}"]
        assert np.array_equal(circles[:, :2], uvs_int[mask])
        assert np.array_equal(circles[:, 2:5], _colours(g, xyzid)[mask])
        assert (circles[:, 5] == int(g["radius"])).all()


def test_golden_filter_masks_follow_the_visibility_rule():
    f = np.load(os.path.join(GOLD, "reproj_filter.npz"), allow_pickle=False)
    for name in (str(n) for n in f["names"]):
        assert np.array_equal(_visible_by_sort(f[f"uv_{name}"], f[f"depth_{name}"]), f[f"mask_{name}"]), name


def test_colormap_lut_matches_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    cmap = matplotlib.colormaps.get_cmap("gist_rainbow")
    lut = RV.colormap_lut("gist_rainbow")
    assert lut.shape == (cmap.N + 3, 3)
    x = np.array([-1.0, -1e-9, 0.0, 0.3, 0.5, 1.0 - 1e-12, 1.0, 1.5, np.nan])
    ref = (cmap(x)[:, :3] * 255).astype(int)
    N = cmap.N
    xa = x * N
    xa[xa == N] = N - 1
    with np.errstate(invalid="ignore"):
        idx = np.where(np.isnan(xa), N + 2, np.where(xa < 0, N, np.where(xa >= N, N + 1, np.nan_to_num(xa).astype(int))))
    assert np.array_equal(lut[idx], ref)
    assert np.array_equal(RV.colormap_lut(cmap), lut) and np.array_equal(RV.colormap_lut(cmap._lut), lut)
    packed, n = RV.pack_lut(lut)
    assert n == N and packed.dtype == np.uint32 and int(packed[5]) == lut[5, 0] | lut[5, 1] << 8 | lut[5, 2] << 16


def test_chunks_bound_the_grid():
    assert RV._chunks([4, 4, 4, 4], 8) == [(0, 2), (2, 4)]
    assert RV._chunks([10, 3, 3], 8) == [(0, 1), (1, 3)]
    assert RV._chunks([5, 5, 5], 1) == [(0, 1), (1, 2), (2, 3)]
    assert RV._chunks([], 8) == []


def test_validation_without_a_device():
    imgs = {"a": np.zeros((10, 12, 3), np.uint8)}
    with pytest.raises(ValueError, match="larger than the video"):
        RV.render(None, None, None, imgs, (11, 10))
    with pytest.raises(NotImplementedError):
        RV.render(None, None, None, imgs, (12, 10), color_mode="dis_to_nowhere")
    with pytest.raises(ValueError, match="draw_radius"):
        RV.render(None, None, None, imgs, (12, 10), draw_radius=-1)
    with pytest.raises(ValueError, match="uint8"):
        RV.render(None, None, None, {"a": np.zeros((10, 12, 3), np.float32)}, (12, 10))


def test_save_video_needs_opencv(monkeypatch):
    monkeypatch.setitem(sys.modules, "cv2", None)
    with pytest.raises(ImportError, match="OpenCV"):
        save_video_with_reprojections("/nonexistent/out.mp4", [np.zeros((4, 4, 3), np.uint8)], (4, 4))


def test_c_abi_entries_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "vggsfm_amd.h")).read()
    for name in ("vgg_reproj_stats_workspace_bytes", "vgg_reproj_stats", "vgg_reproj_visible", "vgg_reproj_draw"):
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.EXPORTED
    assert re.search(r"#define VGG_REPROJ_MAX_RADIUS (\d+)", header).group(1) == str(RV.MAX_RADIUS)
