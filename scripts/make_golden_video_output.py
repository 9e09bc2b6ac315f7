"""Writes tests/golden/video_output_<case>.npz: the output tail of the reference's ``VideoRunner.run`` -- its own
``_update_points_color`` (vggsfm/runners/video_runner.py:475-492), ``dicts_to_output`` (:249-308) with
``dicts_to_reconstruction(extract_color=True)`` (:543-604), ``build_camera_for_video`` (:1019-1049), the rename / rescale
of ``VGGSfMRunner.rename_colmap_recons_and_rescale_camera`` (runner.py:1009-1054) and ``pycolmap_to_batch_matrix`` --
run through oracle.ref_harness with ``pycolmap`` = oracle.pycolmap_shim, on a ``VideoRunner`` made with
``object.__new__`` (as oracle/gen_golden_video.py does) whose ``point_dict`` / ``frame_dict`` hold the state that a
normalising joint BA leaves: points with uint8 zero colours, tracks and per-frame lists in ascending order.

Frames are procedural (tests/video_output_frames.py): the goldens keep the seed, not the pixels.

Cases:
  radial_t60     the last snapshot of tests/golden/video_radial_t60.npz (the reference's own loop): 5,870 points,
                 120,965 observations, 1024 x 1024 frames; back to the original resolution.  The per-image lists are kept
                 as counts and sha256 digests (they are the table's, bit for bit).
  the others     small constructed tables: non-square frames, pixels in (-W, 0) (wrap), just below W, exactly at W, a
                 point whose pixels are all out of range, a point seen once, both camera models, shared_camera and
                 shift_point2d_to_original_res both ways with non-zero crop offsets, back_to_original_resolution both
                 ways, reverse=True on square frames, and two tables the reference raises IndexError on (an index below
                 -W; reverse with the swapped index past H) -- recorded as raises = True.

Run where the reference tree exists:  python scripts/make_golden_video_output.py [case ...]
"""
import hashlib
import os
import sys
import types
import warnings
from collections import defaultdict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import pycolmap_shim, ref_harness  # noqa: E402
from tests.video_output_frames import frames_numpy  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")

# T frames of H x W; crop: the first frame's crop row [real w, real h, ..., top-left x, top-left y, ...] (8 entries).
# Every real size is an exact float32 multiple of H: the reference's resize ratio is a float32 tensor, the port's float64.
CASES = {
    "radial_t60": dict(source="video_radial_t60", seed=101, crop=(1440, 1080, 1, 1, -208.0, 0.0, 0, 0), back=True,
                       shared=True, shift=False, reverse=False),
    "nonsquare_radial": dict(T=6, H=40, W=56, P=90, camera="SIMPLE_RADIAL", seed=202, crop=(100, 60, 1, 1, -14.0, -9.0, 0, 0),
                             back=True, shared=True, shift=True, reverse=False),
    "nonsquare_pinhole_unshared": dict(T=7, H=48, W=36, P=120, camera="SIMPLE_PINHOLE", seed=303,
                                       crop=(72, 96, 1, 1, -6.0, -12.0, 0, 0), back=True, shared=False, shift=False,
                                       reverse=False),
    "radial_unshared_shift": dict(T=5, H=30, W=44, P=70, camera="SIMPLE_RADIAL", seed=404,
                                  crop=(75, 45, 1, 1, -3.0, -7.0, 0, 0), back=True, shared=False, shift=True, reverse=False),
    "square_reverse": dict(T=6, H=40, W=40, P=100, camera="SIMPLE_PINHOLE", seed=505, crop=(80, 80, 1, 1, 0.0, 0.0, 0, 0),
                           back=False, shared=True, shift=False, reverse=True),
    "below_w_raises": dict(T=4, H=32, W=40, P=30, camera="SIMPLE_PINHOLE", seed=606, crop=(80, 64, 1, 1, 0.0, 0.0, 0, 0),
                           back=False, shared=True, shift=False, reverse=False, bad="below_w"),
    "reverse_raises": dict(T=4, H=32, W=40, P=30, camera="SIMPLE_PINHOLE", seed=707, crop=(80, 64, 1, 1, 0.0, 0.0, 0, 0),
                           back=False, shared=True, shift=False, reverse=True, bad="reverse_past_h"),
}


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def constructed_table(c):
    """A point-major observation table (sorted by (point, frame)) with every edge of the index rule in it."""
    rng = np.random.default_rng(c["seed"])
    T, H, W, P = c["T"], c["H"], c["W"], c["P"]
    obs = []
    for p in range(P):
        if p == 0:
            frames = [int(rng.integers(T))]                      # seen once
        else:
            k = int(rng.integers(2, T + 1))
            frames = sorted(rng.choice(T, size=k, replace=False).tolist())
        for f in frames:
            u = rng.uniform(-0.6 * W, 1.15 * W)
            v = rng.uniform(-0.6 * H, 1.15 * H)
            obs.append([p, f, u, v])
    obs = np.array(obs, np.float64)
    uv = obs[:, 2:].astype(np.float32)
    point = obs[:, 0].astype(np.int64)
    # crafted pixels on the first observations of points 1..6
    first = {int(p): int(np.nonzero(point == p)[0][0]) for p in range(1, 7)}
    W32, H32 = np.float32(W), np.float32(H)
    uv[first[1]] = [np.nextafter(W32, np.float32(0)), np.float32(0.5)]          # just below W: included
    uv[first[2]] = [W32, np.float32(1.25)]                                       # exactly W: excluded
    uv[first[3]] = [np.float32(-W + 0.5), np.float32(-0.25)]                     # in (-W, 0): wraps
    uv[first[4]] = [np.float32(2.5), np.nextafter(H32, np.float32(0))]           # just below H
    uv[first[5]] = [np.float32(-0.5), H32]                                       # exactly H: excluded
    sel = point == 6                                                             # every pixel out of range
    uv[sel] = np.stack([np.full(sel.sum(), W + 3.0), np.linspace(-2.0, H + 2.0, sel.sum())], 1).astype(np.float32)
    if c.get("bad") == "below_w":
        uv[first[3]] = [np.float32(-W - 1.5), np.float32(2.0)]                   # u = -W - 2: IndexError
    if c.get("bad") == "reverse_past_h":
        uv[first[1]] = [np.float32(H + 2.5), np.float32(3.0)]                    # u < W but u >= H: IndexError reversed
    frame = obs[:, 1].astype(np.int64)
    xyz = rng.normal(size=(P, 3)).astype(np.float32).astype(np.float64) * 3.0
    q, _ = np.linalg.qr(rng.normal(size=(T, 3, 3)))
    extri = np.concatenate([q, rng.normal(size=(T, 3, 1))], axis=2)
    f = 1.2 * max(H, W)
    K = np.array([[[f, 0, W / 2 + 0.5], [0, f, H / 2 - 0.25], [0, 0, 1]]], np.float32).astype(np.float64)
    extra = np.array([[0.013 if c["camera"] == "SIMPLE_RADIAL" else 0.0]], np.float32).astype(np.float64)
    return dict(obs_point=point, obs_frame=frame, obs_uv=uv, xyz=xyz, extri=extri, intrinsics=K, extra=extra)


def snapshot_table(name):
    g = np.load(os.path.join(OUT, f"{name}.npz"), allow_pickle=False)
    i = int(g["num_snapshots"]) - 1
    tab = dict(obs_point=g[f"s{i}_obs_point"].astype(np.int64), obs_frame=g[f"s{i}_obs_frame"].astype(np.int64),
               obs_uv=g[f"s{i}_obs_uv"], xyz=g[f"s{i}_xyz"].astype(np.float64), extri=g[f"s{i}_extri"],
               intrinsics=g[f"s{i}_intrinsics"], extra=g[f"s{i}_extra"])
    return tab, int(g["T"]), 1024, 1024, str(g["camera_type"]), i


def make_runner(VR, tab, images, c, camera):
    T, H, W = images.shape[1], images.shape[-2], images.shape[-1]
    runner = object.__new__(VR.VideoRunner)
    runner.cfg = types.SimpleNamespace(camera_type=camera, shared_camera=c["shared"], extra_pt_pixel_interval=-1,
                                       shift_point2d_to_original_res=c["shift"])
    runner.device = "cpu"
    runner.images = images
    runner.image_paths = [f"/data/seq/frame_{t:04d}.jpg" for t in range(T)]
    crop = torch.tensor(c["crop"], dtype=torch.float32)[None, None].expand(1, T, -1).clone()
    runner.crop_params = crop[:, 0:1].clone()
    runner.image_size = torch.tensor([W, H], dtype=torch.float32)
    runner.intrinsics = torch.from_numpy(tab["intrinsics"]).float()
    runner.extra_params = torch.from_numpy(tab["extra"]).float()
    runner.point_dict, runner.frame_dict = {}, defaultdict(dict)
    P = len(tab["xyz"])
    for p in range(P):
        runner.point_dict[p] = {"id": p, "xyz": torch.from_numpy(tab["xyz"][p]).float(), "rgb": torch.zeros(3, dtype=torch.uint8),
                                "track": {}}
    for f in range(T):
        runner.frame_dict[f]["extri"] = torch.from_numpy(tab["extri"][f])
        runner.frame_dict[f]["visible_points"] = []
    for p, f, uv in zip(tab["obs_point"].tolist(), tab["obs_frame"].tolist(), tab["obs_uv"]):
        runner.point_dict[p]["track"][f] = {"uv": torch.from_numpy(np.array(uv, np.float32)), "vis": torch.ones(1)}
        runner.frame_dict[f]["visible_points"].append(p)
    return runner


def run_case(name):
    c = CASES[name]
    sys.modules["pycolmap"] = pycolmap_shim
    sys.modules["pyceres"] = pycolmap_shim.pyceres
    ref_harness.install()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import vggsfm.runners.video_runner as VR
    VR.pycolmap, VR.pyceres = pycolmap_shim, pycolmap_shim.pyceres
    if "source" in c:
        tab, T, H, W, camera, snap = snapshot_table(c["source"])
    else:
        tab, T, H, W, camera, snap = constructed_table(c), c["T"], c["H"], c["W"], c["camera"], -1
    images = torch.from_numpy(frames_numpy(c["seed"], 0, T, H, W))[None]
    runner = make_runner(VR, tab, images, c, camera)
    out = dict(case=name, T=np.int64(T), H=np.int64(H), W=np.int64(W), seed=np.int64(c["seed"]), camera_type=camera,
               crop=np.array(c["crop"], np.float32), back=c["back"], shared=c["shared"], shift=c["shift"],
               reverse=c["reverse"], image_paths=np.array(runner.image_paths))
    if "source" in c:
        out.update(source=c["source"], source_snapshot=np.int64(snap), table_sha256=_sha(tab["obs_uv"]))
    else:
        out.update({f"in_{k}": v for k, v in tab.items()})
    try:
        with torch.no_grad():
            runner._update_points_color(reverse=c["reverse"])
    except IndexError as e:
        print(name, "raises IndexError:", e)
        out["raises"] = True
        return out
    out["raises"] = False
    P = len(tab["xyz"])
    rgb = np.zeros((P, 3), np.float32)
    has = np.zeros(P, bool)
    for p in range(P):
        v = runner.point_dict[p]["rgb"]
        if v.dtype == torch.float32:
            rgb[p], has[p] = v.numpy(), True
    out["rgb"], out["has_color"] = rgb, has
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pred = runner.dicts_to_output(0, T, back_to_original_resolution=c["back"])
    rec = pred["reconstruction"]
    pids = sorted(rec.points3D)
    out["point_ids"] = np.array(pids, np.int64)
    out["point_xyz"] = np.stack([rec.points3D[p].xyz for p in pids])
    out["point_color"] = np.stack([np.asarray(rec.points3D[p].color) for p in pids]).astype(np.uint8)
    cams = sorted(rec.cameras)
    out["camera_ids"] = np.array(cams, np.int64)
    out["camera_model"] = np.array([rec.cameras[k].model for k in cams])
    out["camera_wh"] = np.array([[int(rec.cameras[k].width), int(rec.cameras[k].height)] for k in cams], np.int64)
    out["camera_params"] = np.stack([np.asarray(rec.cameras[k].params, np.float64) for k in cams])
    ims = sorted(rec.images)
    out["image_ids"] = np.array(ims, np.int64)
    out["image_names"] = np.array([rec.images[i].name for i in ims])
    out["image_camera"] = np.array([rec.images[i].camera_id for i in ims], np.int64)
    out["image_registered"] = np.array([bool(rec.images[i].registered) for i in ims])
    out["image_pose"] = np.stack([rec.images[i].cam_from_world.matrix() for i in ims])
    counts = np.array([len(rec.images[i].points2D) for i in ims], np.int64)
    p2d_ids = np.concatenate([[p.point3D_id for p in rec.images[i].points2D] for i in ims]).astype(np.int64)
    p2d_xy = np.concatenate([np.array([p.xy for p in rec.images[i].points2D], np.float64).reshape(-1, 2) for i in ims])
    out["p2d_counts"] = counts
    if "source" in c:
        out["p2d_ids_sha256"], out["p2d_xy_sha256"] = _sha(p2d_ids), _sha(p2d_xy)
    else:
        out["p2d_ids"], out["p2d_xy"] = p2d_ids, p2d_xy
    out["pred_extrinsics"] = pred["extrinsics_opencv"].numpy()
    out["pred_intrinsics"] = pred["intrinsics_opencv"].numpy()
    if pred["extra_params"] is not None:
        out["pred_extra_params"] = pred["extra_params"].numpy()
    out["pred_points3D"] = pred["points3D"].numpy()
    out["pred_points3D_rgb"] = pred["points3D_rgb"].numpy()
    assert pred["points3D"].dtype == torch.float32 and pred["points3D_rgb"].dtype == torch.float32
    assert all(pred[k] is None for k in ("unproj_dense_points3D", "valid_2D_mask", "pred_track", "pred_vis", "pred_score",
                                         "valid_tracks"))
    # (rgb * 255 within 1e-4 of a .5: where a float32 sum in another order could round the other way)
    frac = np.abs((rgb[has].astype(np.float64) * 255) % 1.0 - 0.5)
    out["near_half"] = np.int64((frac < 1e-4).sum())
    print(f"{name}: T {T}, {H}x{W}, points {P} ({has.sum()} coloured), observations {len(tab['obs_point'])}, "
          f"cameras {len(cams)} params {out['camera_params'][0]}, near .5: {int(out['near_half'])}")
    return out


def main():
    only = sys.argv[1:]
    for name in CASES:
        if only and name not in only:
            continue
        out = run_case(name)
        path = os.path.join(OUT, f"video_output_{name}.npz")
        np.savez_compressed(path, **out)
        print("wrote", path, f"{os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
