"""GPU times of the track video (vggsfm_amd/track_video.py) on synthetic tracks; writes profiles/track_video_times.json.
Two shapes: the runner's (T = 25 frames of 1024 x 1024, N = 3 x 2048 tracks) and configs[2]'s (T = 200, N = 100,000),
float32 frames on the device, float visibility scores with a fifth of them zero, linewidth 1 (radius 2).  Per shape: the
warm wall time of ``render`` (median of --reps runs, each ended by a device synchronise), and the two entries alone
between device events.  Run each invocation under its own time limit, e.g.
    timeout -k 10 600 python scripts/time_track_video.py
Per-kernel times come from a separate run under the profiler, one shape at a time,
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o tv -- python scripts/time_track_video.py --trace-run --shapes S
whose DIR/**/tv_kernel_stats.csv is merged with  python scripts/time_track_video.py --kernel-stats CSV --shapes S.
The byte and atomic counts printed beside the times are computed here from the shapes and the tracks."""
import argparse
import csv
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"runner": dict(T=25, N=3 * 2048), "configs2": dict(T=200, N=100000)}
SIZE = 1024


def inputs(T, N, seed=0):
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    video = torch.rand((1, T, 3, SIZE, SIZE), generator=gen, device="cuda") * 255
    # a track wanders around its first position, as a tracker's prediction does
    start = torch.rand((1, 1, N, 2), generator=gen, device="cuda") * SIZE
    tracks = start + torch.randn((1, T, N, 2), generator=gen, device="cuda").cumsum(1) * 2.0
    vis = torch.rand((1, T, N, 1), generator=gen, device="cuda")
    vis[vis < 0.2] = 0.0
    return video, tracks, vis


def counts(tracks, vis, out):
    """What the kernels have to do, from the shapes and the tracks: stencil pixels inside the frame (= the most atomics
    the owner pass can issue), bytes of the resolve pass."""
    from vggsfm_amd import track_video as TV
    T, N = tracks.shape[1], tracks.shape[2]
    xy = tracks[0].long()
    inside = ((xy >= 2) & (xy < SIZE - 2)).all(-1) & (xy != 0).all(-1)
    filled = (vis[0, :, :, 0] != 0) & inside
    outline = (vis[0, :, :, 0] == 0) & inside
    pixels = int(filled.sum()) * int(TV.stencil(2, True).sum()) + int(outline.sum()) * int(TV.stencil(2, False).sum())
    px = T * SIZE * SIZE
    return {"circles": T * N, "circles_inside": int(inside.sum()), "stencil_pixels_inside": pixels,
            "resolve_bytes": px * (12 + 4) + int(out.numel()), "owner_clear_bytes": px * 4}


def gpu(a):
    import torch

    from vggsfm_amd import _lib
    from vggsfm_amd import track_video as TV

    res = {"frame": SIZE, "linewidth": 1, "radius": 2, "reps": a.reps, "shapes": {}}
    for name in a.shapes:
        T, N = SHAPES[name]["T"], SHAPES[name]["N"]
        video, tracks, vis = inputs(T, N)
        out = TV.render(video, tracks, vis)                      # warm-up (code objects, allocator)
        torch.cuda.synchronize()
        if a.trace_run:
            for _ in range(RENDERS_PER_TRACE - 1):
                TV.render(video, tracks, vis)
            torch.cuda.synchronize()
            continue
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out2 = TV.render(video, tracks, vis)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        assert torch.equal(out, out2), "two runs differ"
        r = {"T": T, "N": N, "render_ms_median": statistics.median(wall), "render_ms_min": min(wall), "render_ms_max": max(wall)}
        r.update(counts(tracks, vis, out))
        # the two entries alone, one chunk of frames (as render chunks them), between device events
        L, p = _lib.lib(), _lib.ptr
        n = min(T, TV.MAX_GRID_CELLS // (SIZE * SIZE))
        trk, v = tracks[0].contiguous(), vis.reshape(T, N).contiguous()
        owner = torch.empty(n * SIZE * SIZE, dtype=torch.int32, device="cuda")
        colors = torch.from_numpy(TV.rainbow_colors(trk[0, :, 1].long().cpu().numpy()).view(np.int32)).cuda()
        rows = np.array(TV.FILLED_ROWS[2] + TV.OUTLINE_ROWS[2], np.uint32)
        ci, cl = ctypes.c_int, ctypes.c_long
        frames = video[0, :n].contiguous()

        def owner_pass():
            _lib.check(L.vgg_track_owner(p(trk), ci(0), p(v), ci(TV.VIS_F32), ci(0), ci(n), ci(0), cl(N), ci(0), ci(SIZE), ci(SIZE),
                                         ci(2), rows.ctypes.data_as(ctypes.c_void_p), p(owner), _lib.stream_ptr()), "owner")

        def resolve_pass():
            _lib.check(L.vgg_track_resolve(p(frames), ci(0), ci(0), ci(n), ci(SIZE), ci(SIZE), ci(0), p(owner), p(colors), ci(0),
                                           ci(3), p(out), _lib.stream_ptr()), "resolve")
        for label, fn in (("owner_entry", owner_pass), ("resolve_entry", resolve_pass)):
            fn()
            ts = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            r[f"{label}_ms_per_{n}_frames"] = statistics.median(ts)
        r["chunk_frames"] = n
        res["shapes"][name] = r
        print(name, json.dumps(r))
        del video, tracks, vis, out, out2, owner, frames
        torch.cuda.empty_cache()
    return res


RENDERS_PER_TRACE = 4            # --trace-run: the warm-up and three more


def kernel_stats(path):
    """The track-video launches (and the owner grid's clears) of a rocprofv3 kernel_stats.csv of one --trace-run."""
    rows = {}
    for r in csv.DictReader(open(path)):
        name = r["Name"].replace("(anonymous namespace)::", "")
        if "track_" in name or "fillBuffer" in name:
            short = name.split("(")[0].replace("void ", "")
            rows[short] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 2),
                           "ms_per_render": round(float(r["TotalDurationNs"]) / 1e6 / RENDERS_PER_TRACE, 4)}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--trace-run", action="store_true", help="warm-up + 3 renders per shape and no file: for the profiler")
    ap.add_argument("--kernel-stats", metavar="CSV", help="merge a rocprofv3 kernel_stats.csv of a --trace-run into the file")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_video_times.json"))
    a = ap.parse_args()
    old = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.kernel_stats:
        if len(a.shapes) != 1 or a.shapes[0] not in old.get("shapes", {}):
            ap.error("--kernel-stats: name the one shape of the trace run with --shapes, after the timing run of that shape")
        old["shapes"][a.shapes[0]]["kernels"] = {
            "source": f"rocprofv3 --kernel-trace --stats of --trace-run --shapes {a.shapes[0]} ({RENDERS_PER_TRACE} renders)",
            **kernel_stats(a.kernel_stats)}
        res = old
    else:
        res = gpu(a)
        if a.trace_run:
            return
        old.update(res)
        res = old
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
