"""Writes tests/golden/reproj_video_<case>.npz and tests/golden/reproj_filter.npz: the reference's reprojection video
(``create_video_with_reprojections``, vggsfm/utils/utils.py:428-546) and its visibility mask
(``filter_invisible_reprojections``, utils.py:393-425), run through oracle.ref_harness.

OpenCV is not available, so the reference module's ``cv2`` is replaced by a recording stand-in: ``cvtColor`` flips the
channels, ``copyMakeBorder`` is ``np.pad`` (offsets recorded), ``circle`` appends (x, y, colour, radius) to the frame's draw
list.  Everything the reference decides -- colour statistics, colours, centres, the visible set and the drawing order --
is therefore recorded exactly; only OpenCV's anti-aliased raster is not.  The input is the reference's own
``extract_sparse_depth_and_point_from_reconstruction`` (runner.py:744-772) on a ``pycolmap_compat.Reconstruction`` built
from a ``vggsfm_amd.scene`` scene with its cameras scaled to small images, so that pixels collide.  The colour
statistics are restated here with the reference's numpy expressions (utils.py:470-485) on the same points array.

Case features: all three colour modes, two colormaps, draw_radius 0 / 1 / 3 / 5, frames of different sizes (padding),
many pixel collisions, an exactly duplicated point (depth ties), observations off the image on every side (principal
point shifted, images cropped), deleted points (point ids with gaps), an image with no observations (the reference
raises IndexError on it: recorded with the flag ``empty_raises``, its expected frame is the undrawn padded image) and a
single-point model (max_dis == min_dis: NaN colour index, the colormap's "bad" colour).

Run where the reference tree exists:  python scripts/make_golden_reproj_video.py
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402
from vggsfm_amd import pycolmap_compat as pc  # noqa: E402
from vggsfm_amd.scene import make_scene  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")

# name: dict(S, N, camera, shared, seed, scale (1024 px -> 1024/scale), principal-point shift, focal zoom, image sizes (h, w),
#            video (W, H), radius, cmap, mode, duplicate a point, delete ids, empty image)
CASES = {
    "center_r3": dict(S=5, N=300, camera="SIMPLE_PINHOLE", shared=False, seed=3, scale=16.0, pp=(-5.0, -4.0), zoom=1.7,
                      sizes=[(56, 60), (64, 64), (50, 58), (60, 52), (58, 48)], video=(66, 65), radius=3,
                      cmap="gist_rainbow", mode="dis_to_center", dup=True, delete=(), empty=True),
    "origin_r1": dict(S=4, N=600, camera="SIMPLE_RADIAL", shared=True, seed=5, scale=32.0, pp=(-2.0, -3.0), zoom=1.6,
                      sizes=[(30, 32), (32, 28), (26, 30), (32, 32)], video=(34, 33), radius=1, cmap="viridis",
                      mode="dis_to_origin", dup=True, delete=(), empty=False),
    "order_r5": dict(S=4, N=200, camera="SIMPLE_PINHOLE", shared=False, seed=7, scale=16.0, pp=(-3.0, -3.0), zoom=1.6,
                     sizes=[(64, 64), (60, 62), (54, 64), (64, 56)], video=(64, 64), radius=5, cmap="gist_rainbow",
                     mode="point_order", dup=False, delete=(2, 17, 40), empty=False),
    "center_r0": dict(S=3, N=800, camera="SIMPLE_PINHOLE", shared=True, seed=9, scale=32.0, pp=(-1.0, -1.0), zoom=1.5,
                      sizes=[(32, 32), (28, 30), (31, 27)], video=(32, 32), radius=0, cmap="viridis",
                      mode="dis_to_center", dup=True, delete=(), empty=False),
    "single_point": dict(S=3, N=1, camera="SIMPLE_PINHOLE", shared=False, seed=11, scale=16.0, pp=(0.0, 0.0),
                         sizes=[(64, 64), (60, 60), (62, 58)], video=(64, 64), radius=3, cmap="gist_rainbow",
                         mode="dis_to_center", dup=False, delete=(), empty=False),
}


def build_reconstruction(c):
    """The compat reconstruction of case `c`, and the scene arrays it was built from (tests rebuild it from these)."""
    sc = make_scene(c["S"], c["N"], c["camera"], shared_camera=c["shared"], seed=c["seed"], full_visibility=c["N"] == 1)
    pts, tracks, mask = sc.points3D, sc.tracks, sc.mask
    if c["dup"]:                                            # an exact copy of point 0 (same track): depth ties
        pts = np.concatenate([pts, pts[:1]])
        tracks = np.concatenate([tracks, tracks[:, :1]], axis=1)
        mask = np.concatenate([mask, mask[:, :1]], axis=1)
    arrays = dict(points3D=pts, extrinsics=sc.extrinsics, intrinsics=sc.intrinsics, tracks=tracks, mask=mask,
                  extra_params=sc.extra_params if sc.extra_params is not None else np.zeros((0, 1)))
    return rebuild(arrays, c), arrays


def rebuild(a, c):
    extra = a["extra_params"] if c["camera"] == "SIMPLE_RADIAL" else None
    rec = pc.Reconstruction.from_arrays(a["points3D"], a["extrinsics"], a["intrinsics"], a["tracks"], a["mask"],
                                        np.array([1024, 1024]), shared_camera=c["shared"], camera_type=c["camera"],
                                        extra_params=extra)
    for cam in rec.cameras.values():
        cam._params[:3] /= c["scale"]
        cam._params[0] *= c.get("zoom", 1.0)                # spreads the projections past every side of the image
        cam._params[1] += c["pp"][0]
        cam._params[2] += c["pp"][1]
    for pid in c["delete"]:
        rec.delete_point3D(pid)
    if c["empty"]:
        cam = next(iter(rec.cameras.values()))
        rec.add_image(pc.Image(c["S"], f"image_{c['S']}", cam.camera_id, rec.images[0].cam_from_world))
    return rec


class RecordingCV2:
    COLOR_RGB2BGR = 4
    LINE_AA = 16
    BORDER_CONSTANT = 0

    def __init__(self):
        self.frames = []

    def cvtColor(self, img, code):
        assert code == self.COLOR_RGB2BGR
        out = np.ascontiguousarray(img[..., ::-1])
        self.frames.append(dict(circles=[], pad=(0, 0, 0, 0)))
        return out

    def circle(self, img, center, radius, color, thickness, lineType):
        assert thickness == -1 and lineType == self.LINE_AA
        self.frames[-1]["circles"].append((int(center[0]), int(center[1]), *[int(v) for v in color], int(radius)))

    def copyMakeBorder(self, img, top, bottom, left, right, borderType, value):
        assert borderType == self.BORDER_CONSTANT and list(value) == [0, 0, 0]
        self.frames[-1]["pad"] = (top, bottom, left, right)
        return np.pad(img, ((top, bottom), (left, right), (0, 0)))

    def imread(self, *a, **k):
        raise AssertionError("the goldens pass original_images")


def reference_stats(rec, mode):
    """utils.py:470-485 verbatim on the same points array: [median x, y, z, min_dis, max_dis, max id]."""
    points3D = np.array([point.xyz for point in rec.points3D.values()])
    out = np.zeros(8)
    with np.errstate(all="ignore"):
        if mode == "dis_to_center":
            median_point = np.median(points3D, axis=0)
            distances = np.linalg.norm(points3D - median_point, axis=1)
            out[:3] = median_point
            out[3], out[4] = distances.min(), np.percentile(distances, 95)
        elif mode == "dis_to_origin":
            distances = np.linalg.norm(points3D, axis=1)
            out[3], out[4] = distances.min(), distances.max()
        else:
            out[5] = max(rec.point3D_ids())
    return out


def run_case(name):
    c = CASES[name]
    ref_harness.install()
    sys.modules["pycolmap"] = pc
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import matplotlib
        from vggsfm.runners import runner as R
        from vggsfm.utils import utils as U

    rec, arrays = build_reconstruction(c)
    runner = object.__new__(R.VGGSfMRunner)
    pred = runner.extract_sparse_depth_and_point_from_reconstruction({"reconstruction": rec})
    sparse_depth, sparse_point = pred["sparse_depth"], pred["sparse_point"]
    names = sorted(rec.images[i].name for i in rec.images)
    keys = list(sparse_depth)            # (before the reference's second call adds an empty entry to the defaultdict)
    rng = np.random.default_rng(c["seed"])
    rgb = {n: rng.integers(0, 256, size=(*c["sizes"][k % len(c["sizes"])], 3), dtype=np.uint8)
           for k, n in enumerate(names)}
    drawn = [n for n in names if n in sparse_depth]
    rec_cv2 = RecordingCV2()
    saved = U.cv2
    U.cv2 = rec_cv2
    try:
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            frames = U.create_video_with_reprojections("", c["video"], rec, drawn, sparse_depth, sparse_point,
                                                       original_images=rgb, draw_radius=c["radius"], cmap=c["cmap"],
                                                       color_mode=c["mode"])
            empty_raises = False
            if len(drawn) < len(names):
                try:
                    U.create_video_with_reprojections("", c["video"], rec, names, sparse_depth, sparse_point,
                                                      original_images=rgb, draw_radius=c["radius"], cmap=c["cmap"],
                                                      color_mode=c["mode"])
                except IndexError:
                    empty_raises = True
                else:
                    raise AssertionError("the reference drew an image without observations")
    finally:
        U.cv2 = saved
    rec_frames = rec_cv2.frames[:len(drawn)]
    cmap = matplotlib.colormaps.get_cmap(c["cmap"])
    cmap._init()
    xyz_live = np.array([p.xyz for p in rec.points3D.values()]).reshape(-1, 3)
    ids_live = np.array(list(rec.points3D.keys()), np.int64)
    out = dict(case=name, names=np.array(names), drawn=np.array(drawn), keys=np.array(keys), video=np.array(c["video"]),
               radius=c["radius"], cmap=c["cmap"], mode=c["mode"], lut=np.asarray(cmap._lut, np.float64),
               stats=reference_stats(rec, c["mode"]), empty_raises=empty_raises, camera=c["camera"], shared=c["shared"],
               scale=c["scale"], zoom=c.get("zoom", 1.0), pp=np.array(c["pp"]), delete=np.array(c["delete"], np.int64).reshape(-1),
               empty=c["empty"], points_xyz=xyz_live, point_ids=ids_live, **arrays)
    for j, k in enumerate(keys):
        out[f"uvd_{j}"] = np.array(sparse_depth[k])
        out[f"xyzid_{j}"] = np.array(sparse_point[k])
    for k, n in enumerate(names):
        out[f"rgb_{k}"] = rgb[n]
    for k, n in enumerate(drawn):
        f, img = rec_frames[k], frames[k]
        circles = np.array(f["circles"], np.int64).reshape(-1, 6)
        out[f"circles_{drawn.index(n)}"] = circles
        out[f"pad_{drawn.index(n)}"] = np.array(f["pad"], np.int64)
        assert img.shape == (c["video"][1], c["video"][0], 3)
    # off the image on all four sides (over the case's frames)
    sides = np.zeros(4, bool)
    for n in drawn:
        uv = np.round(np.array(sparse_depth[n])[:, :2])
        h, w = rgb[n].shape[:2]
        sides |= [(uv[:, 0] < 0).any(), (uv[:, 0] >= w).any(), (uv[:, 1] < 0).any(), (uv[:, 1] >= h).any()]
    out["off_sides"] = sides
    return out


def filter_cases():
    """Crafted inputs of filter_invisible_reprojections and the reference's masks."""
    ref_harness.install()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from vggsfm.utils import utils as U
    rng = np.random.default_rng(0)
    cases = {}
    # negative coordinates, ties, +-0.0, NaN and negative depths
    uv = np.array([[-3, -1], [-3, -1], [0, 0], [0, 0], [0, 0], [5, -7], [5, -7], [2, 2], [2, 2], [2, 2], [-1, 4],
                   [-1, 4], [9, 9], [9, 9], [9, 9], [-2, -2], [-2, -2]], np.int64)
    d = np.array([2.0, 2.0, 0.0, -0.0, 1.0, -3.0, -1.0, 1.0, np.nan, np.nan, -0.0, 0.0, 4.0, np.nan, -np.inf, np.inf,
                  np.inf])
    cases["crafted"] = (uv, d)
    # random pixels of a small frame, many collisions, a few exact ties
    uv = rng.integers(-20, 20, size=(3000, 2))
    d = np.round(rng.uniform(-1.0, 5.0, size=3000), 1)
    cases["collisions"] = (uv, d)
    # a sparse extent that is wide but within the device grid's cell limit (2^27)
    uv = np.concatenate([rng.integers(-9000, 9000, size=(400, 1)), rng.integers(-800, 800, size=(400, 1))], axis=1)
    uv = np.concatenate([uv, uv[:50]])
    d = rng.uniform(0.5, 2.0, size=450)
    cases["wide"] = (uv, d)
    out = {}
    for k, (uv, d) in cases.items():
        out[f"uv_{k}"], out[f"depth_{k}"] = uv, d
        out[f"mask_{k}"] = U.filter_invisible_reprojections(uv, d)
    # beyond the limit: only the input (the device side raises ValueError; the reference would loop over it)
    out["uv_too_wide"] = np.array([[-20000, -20000], [20000, 20000], [0, 0]], np.int64)
    out["depth_too_wide"] = np.array([1.0, 2.0, 3.0])
    out["names"] = np.array(list(cases))
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    total = 0
    for name in CASES:
        out = run_case(name)
        path = os.path.join(OUT, f"reproj_video_{name}.npz")
        np.savez_compressed(path, **out)
        total += os.path.getsize(path)
        ncirc = [len(out[f"circles_{k}"]) for k in range(len(out["drawn"]))]
        nobs = [len(out[f"uvd_{j}"]) for j in range(len(out["keys"]))]
        print(f"{path}: observations {nobs}, circles {ncirc}, off left/right/top/bottom {out['off_sides']}, stats {out['stats'][:6]}, "
              f"{os.path.getsize(path) / 1e3:.0f} kB")
    path = os.path.join(OUT, "reproj_filter.npz")
    np.savez_compressed(path, **filter_cases())
    total += os.path.getsize(path)
    print(f"{path}: {os.path.getsize(path) / 1e3:.0f} kB; all {total / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
