"""The reprojection video on the MI355X against the reference's create_video_with_reprojections and
filter_invisible_reprojections (utils.py:393-546), recorded in tests/golden/reproj_video_*.npz / reproj_filter.npz by
scripts/make_golden_reproj_video.py (OpenCV's circle calls captured: centre, colour, radius, order)."""
import os

import numpy as np
import pytest
import torch

from vggsfm_amd import dense_depth as DD
from vggsfm_amd import pycolmap_compat as pc
from vggsfm_amd import reproj_video as RV
from vggsfm_amd.runners import GeometryConfig, GeometryRunner
from vggsfm_amd.utils.utils import create_video_with_reprojections, filter_invisible_reprojections

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["center_r3", "origin_r1", "order_r5", "center_r0", "single_point"]


def _golden(case):
    return np.load(os.path.join(GOLD, f"reproj_video_{case}.npz"), allow_pickle=False)


def _strs(a):
    return [str(n) for n in a]


def _sparse_depth(g):
    keys = _strs(g["keys"])
    uvd = [g[f"uvd_{j}"] for j in range(len(keys))]
    xyzid = [g[f"xyzid_{j}"] for j in range(len(keys))]
    obs_ptr = np.concatenate([[0], np.cumsum([len(u) for u in uvd])]).astype(np.int64)
    return DD.SparseDepth(keys, obs_ptr, torch.from_numpy(np.concatenate(uvd)).cuda(),
                          torch.from_numpy(np.concatenate(xyzid)).cuda())


def _images(g):
    return {n: g[f"rgb_{k}"] for k, n in enumerate(_strs(g["names"]))}


def _reconstruction(g):
    """The compat reconstruction the golden script built (scaled, zoomed and shifted cameras, deleted points, empty image)."""
    camera, shared = str(g["camera"]), bool(g["shared"])
    extra = g["extra_params"] if camera == "SIMPLE_RADIAL" else None
    rec = pc.Reconstruction.from_arrays(g["points3D"], g["extrinsics"], g["intrinsics"], g["tracks"], g["mask"],
                                        np.array([1024, 1024]), shared_camera=shared, camera_type=camera,
                                        extra_params=extra)
    for c in rec.cameras.values():
        c._params[:3] /= float(g["scale"])
        c._params[0] *= float(g["zoom"])
        c._params[1] += float(g["pp"][0])
        c._params[2] += float(g["pp"][1])
    for pid in g["delete"]:
        rec.delete_point3D(int(pid))
    if bool(g["empty"]):
        cam = next(iter(rec.cameras.values()))
        S = len(rec.images)
        rec.add_image(pc.Image(S, f"image_{S}", cam.camera_id, rec.images[0].cam_from_world))
    return rec


def _coverage(a, b, r):
    """The raster rule: 4 x 4 sub-samples at (2i - 3) / 8 inside the disc; r = 0: the centre pixel."""
    if r == 0:
        return np.where((a == 0) & (b == 0), 16, 0)
    k = np.zeros(np.broadcast(a, b).shape, np.int64)
    for i in range(4):
        for j in range(4):
            k += ((8 * a + 2 * i - 3) ** 2 + (8 * b + 2 * j - 3) ** 2 <= 64 * r * r)
    return k


def _composite(bgr, circles):
    """numpy restatement of the compositing: every recorded circle, in the recorded order."""
    out = bgr.astype(np.int64)
    h, w = out.shape[:2]
    for x, y, c0, c1, c2, r in circles:
        y0, y1, x0, x1 = max(0, y - r), min(h, y + r + 1), max(0, x - r), min(w, x + r + 1)
        if y0 >= y1 or x0 >= x1:
            continue
        ys, xs = np.mgrid[y0:y1, x0:x1]
        k = _coverage(xs - x, ys - y, r)[..., None]
        c = np.array([c0, c1, c2], np.int64)
        out[ys, xs] = (out[ys, xs] * (16 - k) + c * k + 8) >> 4
    return out.astype(np.uint8)


def _expected_frames(g):
    """Per name of the video, the reference's padded frame with the recorded draw list composited by the raster rule (an
    image without observations: undrawn, the pad by the reference's rule)."""
    W, H = (int(v) for v in g["video"])
    drawn = _strs(g["drawn"])
    out = []
    for k, n in enumerate(_strs(g["names"])):
        bgr = g[f"rgb_{k}"][..., ::-1]
        h, w = bgr.shape[:2]
        if n in drawn:
            j = drawn.index(n)
            img, pad = _composite(bgr, g[f"circles_{j}"]), g[f"pad_{j}"]
        else:
            top, left = (H - h) // 2, (W - w) // 2
            img, pad = bgr, (top, H - h - top, left, W - w - left)
        out.append(np.pad(img, ((pad[0], pad[1]), (pad[2], pad[3]), (0, 0))))
        assert out[-1].shape == (H, W, 3)
    return out


def _render(g, **kw):
    return RV.render(_sparse_depth(g), g["points_xyz"], g["point_ids"], _images(g), tuple(int(v) for v in g["video"]),
                     draw_radius=int(g["radius"]), cmap=g["lut"], color_mode=str(g["mode"]), **kw)


@pytest.mark.parametrize("case", CASES)
def test_draw_list_and_stats_match_reference(case):
    g = _golden(case)
    r = int(g["radius"])
    _, dbg = _render(g, return_debug=True)
    assert np.array_equal(dbg.stats.cpu().numpy()[:6].view(np.int64), g["stats"][:6].view(np.int64))
    vis, cen, col = dbg.visible.cpu().numpy(), dbg.centers.cpu().numpy(), dbg.colors.cpu().numpy()
    drawn = _strs(g["drawn"])
    for f, n in enumerate(dbg.names):
        if n not in drawn:
            continue
        a, b = dbg.obs_range[f]
        h, w = g[f"rgb_{f}"].shape[:2]
        ref = g[f"circles_{drawn.index(n)}"]
        inwin = (ref[:, 0] >= -r) & (ref[:, 0] < w + r) & (ref[:, 1] >= -r) & (ref[:, 1] < h + r)
        ref = ref[inwin]
        assert (ref[:, 5] == r).all()
        o = np.arange(a, b)[vis[a:b] == 1]                 # observation order = the reference's drawing order
        ours = np.concatenate([cen[o].astype(np.int64), col[o].astype(np.int64)], axis=1)
        assert np.array_equal(ours, ref[:, :5]), (case, n)
        assert len(ref) > 0


@pytest.mark.parametrize("case", CASES)
def test_frames_match_raster_restatement(case):
    g = _golden(case)
    frames = _render(g).cpu().numpy()
    W, H = (int(v) for v in g["video"])
    expected = _expected_frames(g)
    assert frames.shape == (len(expected), H, W, 3) and frames.dtype == np.uint8
    for k, e in enumerate(expected):
        assert np.array_equal(frames[k], e), (case, k, int((frames[k] != e).sum()))


def test_single_point_is_the_bad_colour():
    g = _golden("single_point")
    for j in range(len(g["drawn"])):
        assert np.array_equal(g[f"circles_{j}"][:, 2:5], np.zeros((1, 3), np.int64))
    _, dbg = _render(g, return_debug=True)
    assert (dbg.colors.cpu().numpy() == 0).all()


def test_empty_image_is_output_undrawn():
    g = _golden("center_r3")
    assert bool(g["empty_raises"]) and len(g["drawn"]) < len(g["names"])
    frames = _render(g).cpu().numpy()
    k = _strs(g["names"]).index(next(n for n in _strs(g["names"]) if n not in _strs(g["drawn"])))
    assert np.array_equal(frames[k], _expected_frames(g)[k])


def test_chunked_grids_give_the_same_frames():
    g = _golden("origin_r1")
    whole = _render(g).cpu().numpy()
    one_per_chunk = _render(g, max_grid_cells=1).cpu().numpy()
    assert np.array_equal(whole, one_per_chunk)


def test_filter_invisible_reprojections_matches_reference():
    f = np.load(os.path.join(GOLD, "reproj_filter.npz"), allow_pickle=False)
    for name in _strs(f["names"]):
        uv, d, ref = f[f"uv_{name}"], f[f"depth_{name}"], f[f"mask_{name}"]
        m = filter_invisible_reprojections(uv, d)
        assert isinstance(m, np.ndarray) and m.dtype == bool and np.array_equal(m, ref), name
        md = filter_invisible_reprojections(torch.from_numpy(uv).cuda(), torch.from_numpy(d).cuda())
        assert md.is_cuda and md.dtype == torch.bool and np.array_equal(md.cpu().numpy(), ref), name
    with pytest.raises(ValueError, match="pixels"):
        filter_invisible_reprojections(f["uv_too_wide"], f["depth_too_wide"])


def test_utils_and_runner_match_the_golden_frames():
    g = _golden("center_r3")                  # the reference's defaults: gist_rainbow, radius 3, dis_to_center
    rec = _reconstruction(g)
    runner = GeometryRunner(GeometryConfig())
    pred = runner.extract_sparse_depth_and_point_from_reconstruction({"reconstruction": rec})
    names = _strs(g["names"])
    rgb = _images(g)
    video = tuple(int(v) for v in g["video"])
    host = create_video_with_reprojections("", video, rec, names, pred["sparse_depth"], pred["sparse_point"],
                                           original_images=rgb, cmap=g["lut"])
    assert len(host) == len(names) and all(isinstance(f, np.ndarray) and f.shape == (video[1], video[0], 3) for f in host)
    frames = runner.make_reprojection_video(pred, video, [f"/data/{n}" for n in names], rgb)
    for a, b in zip(frames, host):
        assert np.array_equal(a, b)
    on_dev = runner.make_reprojection_video(pred, video, [f"/data/{n}" for n in names],
                                            {n: torch.from_numpy(v).cuda() for n, v in rgb.items()})
    for a, b in zip(on_dev, host):
        assert np.array_equal(a, b)
    # the projection of the reconstruction is the reference's to well below a pixel: the frames are the golden ones
    # wherever no observation sits within 1e-6 px of a rounding boundary
    expected = _expected_frames(g)
    uv = pred["sparse_depth_device"].uvd[:, :2].cpu().numpy()
    if not (np.abs(np.abs(uv - np.floor(uv)) - 0.5) < 1e-6).any():
        for a, e in zip(host, expected):
            assert np.array_equal(a, e)


def test_repeated_calls_are_bit_identical():
    g = _golden("center_r0")
    a = _render(g).cpu().numpy()
    b = _render(g).cpu().numpy()
    assert np.array_equal(a, b)


def test_validation_before_any_launch():
    g = _golden("center_r3")
    imgs = _images(g)
    video = tuple(int(v) for v in g["video"])
    with pytest.raises(ValueError, match="larger than the video"):
        RV.render(None, None, None, imgs, (video[0] - 10, video[1]), cmap=g["lut"])
    with pytest.raises(NotImplementedError):
        RV.render(None, None, None, imgs, video, cmap=g["lut"], color_mode="dis_to_nowhere")
    with pytest.raises(ValueError, match="draw_radius"):
        RV.render(None, None, None, imgs, video, draw_radius=-1, cmap=g["lut"])
    with pytest.raises(ValueError, match="larger than the video"):
        create_video_with_reprojections("", (8, 8), None, list(imgs), {}, {}, original_images=imgs)
