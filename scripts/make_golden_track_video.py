"""Writes tests/golden/track_video_<case>.npz: the reference's own ``Visualizer.visualize(save_video=False)``
(vggsfm/utils/visualizer.py:87-295) with the real PIL and matplotlib, imported through oracle.ref_harness (imageio and
torchvision are stubbed there; matplotlib >= 3.9 has no ``cm.get_cmap``, which the reference calls, so it is pointed at
``matplotlib.colormaps.get_cmap`` before the import).  Each file holds the inputs -- frames as uint8 values plus the
fraction that is added to them as float32 (so that the truncation is exercised), tracks float32, visibility -- the
options, and the reference's output frames.  The files are written with fixed zip time stamps: the same script gives the
same bytes.

  python scripts/make_golden_track_video.py [case ...]     the goldens (where the reference tree exists)
  python scripts/make_golden_track_video.py --stencils     print PIL's stencil tables of vggsfm_amd/track_video.py and
                                                           compare them with the committed ones
  python scripts/make_golden_track_video.py --time         time the reference's drawing loop on this CPU (two frames of
                                                           1024 x 1024, 20,000 tracks) -> profiles/track_video_reference_cpu.json

Cases (tracks are uniform over the frame and a margin around it, so centres lie off every side and straddle every border
and corner; the first tracks of every frame are crafted: 0.4 and -0.6 truncate to 0 and are skipped, -1.2 and 1.0 are not):
  default          the runner's call: rainbow, linewidth 1, float visibility scores with exact zeros, a -0.0 and a NaN
  cool_lw2_pad3    mode "cool", linewidth 2, an odd pad on an odd width, query_frame 2, show_first_frame 0, bool visibility
  lw3_novis        linewidth 3, no visibility, a width that is no multiple of 4, query_frame 1
  pad4             rainbow with pad_value 4 on a width that is a multiple of 4
  contested        4,000 tracks on 40 x 52 pixels: most pixels are contested
  single_track     one track (y_min == y_max)
  one_frame        T = 1
"""
import io
import json
import os
import sys
import time
import warnings
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")

CASES = {
    "default": dict(T=6, H=64, W=80, N=300, seed=11, mode="rainbow", linewidth=1, pad_value=0, query_frame=0,
                    show_first_frame=3, vis="float"),
    "cool_lw2_pad3": dict(T=5, H=48, W=61, N=400, seed=12, mode="cool", linewidth=2, pad_value=3, query_frame=2,
                          show_first_frame=0, vis="bool"),
    "lw3_novis": dict(T=4, H=50, W=70, N=250, seed=13, mode="rainbow", linewidth=3, pad_value=0, query_frame=1,
                      show_first_frame=3, vis=None),
    "pad4": dict(T=4, H=40, W=64, N=300, seed=14, mode="rainbow", linewidth=1, pad_value=4, query_frame=0,
                 show_first_frame=3, vis="float"),
    "contested": dict(T=4, H=40, W=52, N=4000, seed=15, mode="rainbow", linewidth=1, pad_value=0, query_frame=0,
                      show_first_frame=3, vis="float"),
    "single_track": dict(T=3, H=32, W=36, N=1, seed=16, mode="rainbow", linewidth=1, pad_value=0, query_frame=0,
                         show_first_frame=3, vis="float"),
    "one_frame": dict(T=1, H=32, W=44, N=200, seed=17, mode="rainbow", linewidth=1, pad_value=1, query_frame=0,
                      show_first_frame=3, vis="float"),
}
FRAME_FRAC = 0.75       # frames reach the reference as float32(uint8 value) + 0.75: .byte() must truncate it away


def make_inputs(c):
    rng = np.random.default_rng(c["seed"])
    T, H, W, N = c["T"], c["H"], c["W"], c["N"]
    r = int(c["linewidth"] * 2)
    # smooth frames with some noise (any content serves; this compresses)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([(xx * 3 + yy) % 256, (yy * 5 + 40) % 256, (xx + yy * 2) % 256])
    frames = np.stack([(base + 17 * t + rng.integers(0, 8, size=base.shape)) % 256 for t in range(T)]).astype(np.uint8)
    frames[:, :, 0, 0] = 255                                  # 255.75 stays below 256
    frames[:, :, 0, 1] = 0
    m = r + 3.0
    tracks = np.stack([rng.uniform(-m, W + m, size=(T, N)), rng.uniform(-m, H + m, size=(T, N))], -1).astype(np.float32)
    crafted = [(0.4, 10.3), (10.7, -0.6), (-0.6, 0.4), (-1.2, 5.5), (7.2, -1.2), (1.0, 1.0), (0.999, 20.0), (-0.999, 9.0),
               (W - 1.0, H - 1.0), (W + 0.0, H + 0.0), (W + r - 0.5, 12.0), (13.0, H + r + 0.2), (-r - 0.3, 6.0),
               (6.0, -r - 0.9), (-1.0, -1.0), (W - 0.5, -1.5), (-1.5, H - 0.5), (W / 2, H / 2), (W / 2, H / 2)]
    if N == 1:                                                # the single track stays in sight, and moves
        tracks[:, 0] = [(W / 2 + 2.6 * t, H / 2 - 1.7 * t) for t in range(T)]
    else:
        for k, xy in enumerate(crafted[:N]):
            tracks[:, k] = xy
    tracks[T - 1, min(3, N - 1)] = (1.0e9, 5.0)               # far off the frame
    vis = None
    if c["vis"] == "float":
        vis = rng.uniform(0.0, 1.0, size=(T, N)).astype(np.float32)
        vis[rng.uniform(size=(T, N)) < 0.3] = 0.0
        vis[0, 0] = 0.7
        if N > 20:
            vis[:, 17], vis[:, 18] = 0.0, 0.9                  # an outline under a filled circle at the same centre
            vis[T - 1, 19], vis[0, 20] = np.nan, -0.0
    elif c["vis"] == "bool":
        vis = rng.uniform(size=(T, N)) < 0.7
    return frames, tracks, vis


def reference_visualizer():
    import matplotlib
    from matplotlib import cm
    if not hasattr(cm, "get_cmap"):
        cm.get_cmap = matplotlib.colormaps.get_cmap
    ref_harness.install()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import vggsfm.utils.visualizer as V
    return V


def run_reference(V, c, frames, tracks, vis):
    viz = V.Visualizer(save_dir="unused", mode=c["mode"], linewidth=c["linewidth"], pad_value=c["pad_value"],
                       show_first_frame=c["show_first_frame"])
    video = torch.from_numpy(frames.astype(np.float32) + np.float32(FRAME_FRAC))[None]
    v = None if vis is None else torch.from_numpy(vis)[None, :, :, None]
    out = viz.visualize(video, torch.from_numpy(tracks)[None], v, query_frame=c["query_frame"], save_video=False)
    return out[0].numpy()


def save_npz(path, arrays):
    """np.savez_compressed with fixed time stamps and member order."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def pil_stencil_rows(radius, filled):
    from PIL import Image, ImageDraw
    c, size = 40, 96
    im = Image.new("RGB", (size, size))
    ImageDraw.Draw(im).ellipse([(c - radius, c - radius), (c + radius, c + radius)], fill=(255, 0, 0) if filled else None,
                               outline=(255, 0, 0))
    a = np.array(im)[..., 0] > 0
    box = a[c - radius:c + radius + 1, c - radius:c + radius + 1]
    assert a.sum() == box.sum(), "PIL drew outside the bounding box"
    return tuple(int(sum(1 << int(b) for b in np.nonzero(row)[0])) for row in box)


def stencils():
    import textwrap

    import PIL

    from vggsfm_amd import track_video as TV
    print(f"# Pillow {PIL.__version__}")
    same = True
    for name, filled in (("FILLED_ROWS", True), ("OUTLINE_ROWS", False)):
        print(f"{name} = (")
        for r in range(TV.MAX_RADIUS + 1):
            rows = pil_stencil_rows(r, filled)
            same = same and rows == getattr(TV, name)[r]
            body = ", ".join(f"0x{m:x}" for m in rows)
            for k, line in enumerate(textwrap.wrap(f"({body},),", 112)):
                print("    " + ("" if k == 0 else " ") + line)
        print(")")
    print("# equal to vggsfm_amd/track_video.py:", same)
    return same


def time_reference():
    import PIL
    V = reference_visualizer()
    out = {"what": "the reference's Visualizer.visualize on this CPU (PIL circles in a Python loop), for comparison only",
           "pillow": PIL.__version__, "shapes": []}
    for T, H, W, N in ((2, 1024, 1024, 20000), (2, 64, 80, 20000)):
        rng = np.random.default_rng(5)
        frames = rng.integers(0, 256, size=(T, 3, H, W)).astype(np.uint8)
        tracks = np.stack([rng.uniform(1, W - 1, size=(T, N)), rng.uniform(1, H - 1, size=(T, N))], -1).astype(np.float32)
        vis = rng.uniform(0.1, 1.0, size=(T, N)).astype(np.float32)
        c = dict(mode="rainbow", linewidth=1, pad_value=0, show_first_frame=3, query_frame=0)
        t0 = time.perf_counter()
        run_reference(V, c, frames, tracks, vis)
        dt = time.perf_counter() - t0
        out["shapes"].append({"T": T, "H": H, "W": W, "N": N, "seconds": round(dt, 3),
                              "us_per_circle": round(dt / (T * N) * 1e6, 2)})
        print(out["shapes"][-1])
    per = out["shapes"][0]["us_per_circle"]
    out["extrapolated_configs2_seconds"] = round(per * 1e-6 * 200 * 100000, 1)
    out["note"] = ("extrapolated_configs2_seconds = us_per_circle of the 1024 x 1024 run x 200 frames x 100,000 tracks: an "
                   "extrapolation, not a run, and a CPU figure of the build machine")
    path = os.path.join(ROOT, "profiles", "track_video_reference_cpu.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


def main():
    args = sys.argv[1:]
    if "--stencils" in args:
        sys.exit(0 if stencils() else 1)
    if "--time" in args:
        return time_reference()
    V = reference_visualizer()
    for name, c in CASES.items():
        if args and name not in args:
            continue
        frames, tracks, vis = make_inputs(c)
        expect = run_reference(V, c, frames, tracks, vis)
        arrays = dict(frames=frames, frame_frac=np.float32(FRAME_FRAC), tracks=tracks, expect=expect,
                      mode=np.array(c["mode"]), linewidth=np.int64(c["linewidth"]), pad_value=np.int64(c["pad_value"]),
                      query_frame=np.int64(c["query_frame"]), show_first_frame=np.int64(c["show_first_frame"]))
        if vis is not None:
            arrays["visibility"] = vis
        path = os.path.join(OUT, f"track_video_{name}.npz")
        save_npz(path, arrays)
        pad = c["pad_value"]
        canvas = np.full((c["T"], 3, c["H"] + 2 * pad, c["W"] + 2 * pad), 255, np.uint8)
        canvas[:, :, pad:pad + c["H"], pad:pad + c["W"]] = frames
        first = max(c["show_first_frame"], 1) - 1
        drawn = (expect[first:] != canvas).any(1).mean()
        print(f"{name}: out {expect.shape}, {100 * drawn:.0f} % of the pixels drawn, {os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
