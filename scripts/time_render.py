"""GPU times of the rasteriser's entries (csrc/raster/raster.hip); writes profiles/render_times.json.  Medians of --reps
windows of --inner calls between device events after a warm-up, min .. max beside (the method of scripts/time_mvs.py).

Two workloads, each into 9 views of 512 x 512 (the cameras of scripts/time_fusion.py, in front of the plane z = 4):
  mesh   the mesh of scripts/time_meshing.py: the 9 depth maps integrated into 256^3 nodes and extracted (voxel-sized faces:
         every candidate box is a handful of pixels, walked by its lane alone)
  quad   two triangles that fill every frame (the wave-cooperative path: 64 lanes stride over each box)
Per workload:
  clear          the key buffer filled with -1 (torch), for reference: `raster` below includes it
  raster         clear + vggz_raster: every call draws onto empty keys, so the atomics that a first draw needs are issued
  redraw         vggz_raster onto keys that already hold the result: every candidate is tested, the plain load finds no
                 smaller key to write and no atomic is issued
  resolve        vggz_resolve with every output (depth, face, weights, normals, colours)
and `raster` once more per variant, in builds of the translation unit of this script's own under --build-dir (never the
library): without the plain-load early-out (-DVGGZ_NO_EARLY_OUT: every covered candidate issues its 64-bit atomic minimum --
the price of the atomics) and with other thresholds between the lane-alone walk and the cooperative one
(-DVGGZ_SOLO_OVERRIDE=N; 0 = every face cooperative).
Beside each time: faces per second, covered pixels per second (pixels that hold a key after the draw, over the views) and
candidate pixels (the sum of the faces' box sizes, by the header's box formula restated in torch) per covered pixel.
visibility: vggz_point_visibility of the mesh's vertices against the 9 rendered depth maps.
No thresholds: the numbers are reported; the parent commit has nothing that does this work.  Run under its own time limit:
    timeout -k 10 420 python scripts/time_render.py
"""
import argparse
import ctypes
import json
import math
import os
import platform
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_fusion import scene  # noqa: E402
from time_mvs import windows  # noqa: E402

VARIANTS = (("no_early_out", ["-DVGGZ_NO_EARLY_OUT"]), ("solo_0", ["-DVGGZ_SOLO_OVERRIDE=0"]), ("solo_16", ["-DVGGZ_SOLO_OVERRIDE=16"]),
            ("solo_256", ["-DVGGZ_SOLO_OVERRIDE=256"]), ("solo_4096", ["-DVGGZ_SOLO_OVERRIDE=4096"]))


def build_variant(name, flags, build_dir):
    """the rasteriser's translation unit with extra -D flags -> a loaded library with the table's types"""
    from vggsfm_amd import _lib, _lib_raster as Z
    src = os.path.join(ROOT, "vggsfm_amd", "csrc", "raster", "raster.hip")
    out = os.path.join(build_dir, f"libraster_{name}.so")
    os.makedirs(build_dir, exist_ok=True)
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                           "-munsafe-fp-atomics", "-ffp-contract=off", "-shared", *flags, src, "-o", out])
    L = ctypes.CDLL(out)
    _lib.bind(L, Z.SIGNATURES)
    return L


def candidate_pixels(vertices, faces, poses, cams, near, H, W):
    """the sum over views and faces of the header's box size, in torch on the device (float64)"""
    import torch
    total = 0
    P = vertices[faces.long()]                                               # (F,3,3)
    for s in range(poses.shape[0]):
        R, t = poses[s, :, :3], poses[s, :, 3]
        Xc = P @ R.T + t
        iz = 1.0 / Xc[..., 2]
        a, b = Xc[..., 0] * iz, Xc[..., 1] * iz
        f, cx, cy, k = (float(v) for v in cams[s])
        d = 1.0 + k * (a * a + b * b)
        x, y = f * (a * d) + cx, f * (b * d) + cy
        r = (a * a + b * b).amax(1).sqrt()
        L2 = ((a.roll(-1, 1) - a) ** 2 + (b.roll(-1, 1) - b) ** 2).amax(1)
        m = 1.0 + 0.75 * f * abs(k) * r * L2
        x0, x1 = (x.amin(1) - m).floor().clamp(min=0), (x.amax(1) + m).ceil().clamp(max=W - 1)
        y0, y1 = (y.amin(1) - m).floor().clamp(min=0), (y.amax(1) + m).ceil().clamp(max=H - 1)
        area = (a[:, 1] - a[:, 0]) * (b[:, 2] - b[:, 0]) - (b[:, 1] - b[:, 0]) * (a[:, 2] - a[:, 0])
        ok = (Xc[..., 2] > near).all(1) & (area != 0) & (x1 >= x0) & (y1 >= y0)
        total += int(((x1 - x0 + 1) * (y1 - y0 + 1))[ok].sum().item())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=9)
    ap.add_argument("--nodes", type=int, default=256)
    ap.add_argument("--build-dir", default="/tmp/vggsfm_amd_time_render")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_times.json"))
    a = ap.parse_args()
    import torch
    from vggsfm_amd import _lib_raster as Z
    from vggsfm_amd import meshing, mvs, render
    assert torch.cuda.is_available(), "needs an MI355X"
    prop = torch.cuda.get_device_properties(0)
    S, H, W, near = a.views, a.size, a.size, 1e-6
    res = {"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "memory_gb": round(prop.total_memory / 2 ** 30), "host": platform.node(), "reps": a.reps, "inner": a.inner, "size": a.size,
           "views": S, "nodes_per_side": a.nodes, "solo_pixels": Z.SOLO_PIXELS}
    depth, colors, poses, cams = scene(a.size, S)
    side = 4.0 * a.size / (1.25 * a.size)                                    # the grid of scripts/time_meshing.py
    voxel = side / (a.nodes - 1)
    vol = meshing.TSDFVolume((-side / 2 + 0.013, -side / 2 + 0.007, 4.0 - side / 2 + 0.011), voxel, (a.nodes,) * 3)
    vol.integrate(depth, poses, cams, None, colors, 4.0 * voxel)
    mesh = vol.extract(1.0)
    del vol
    dev = depth.device
    quad_v = torch.tensor([[-3.1, -2.9, 4.0], [3.2, -3.0, 4.1], [3.0, 3.1, 4.2], [-2.9, 3.2, 4.05]], dtype=torch.float64, device=dev)
    quad_f = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32, device=dev)
    quad_n = torch.tensor([[0.0, 0.0, -1.0]] * 4, dtype=torch.float32, device=dev)
    quad_c = torch.rand(4, 3, generator=torch.Generator(device="cuda").manual_seed(1), device=dev)
    rays, ridx = mvs.camera_rays(cams, H, W, dev)
    keys = render.new_keys(S, H, W, dev)
    libs = {"library": Z.lib()}
    for name, flags in VARIANTS:
        libs[name] = build_variant(name, flags, a.build_dir)
    workloads = {"mesh": (mesh.vertices.contiguous(), mesh.faces.contiguous(), mesh.normals.contiguous(), mesh.rgb.contiguous()),
                 "quad": (quad_v, quad_f, quad_n, quad_c)}
    reference = {}
    for wname, (v, f, n, c) in workloads.items():
        V, F = v.shape[0], f.shape[0]
        out = res[wname] = {"vertices": V, "faces": F}

        def draw(L):
            Z.check(L.vggz_raster(v, V, f, F, 0, poses, cams, rays, ridx, rays.shape[0], S, H, W, near, keys, Z.stream_ptr()),
                    "vggz_raster")

        def fresh(L):
            keys.fill_(-1)
            draw(L)
        fresh(libs["library"])
        reference[wname] = keys.clone()
        covered = int((keys != -1).sum().item())
        cand = candidate_pixels(v, f, poses, cams, near, H, W)
        out.update(covered_pixels=covered, candidate_pixels=cand, candidates_per_covered_pixel=cand / max(covered, 1))

        def rate(r):
            s = r["ms_median"] / 1e3
            r.update(faces_per_s=F * S / s, covered_pixels_per_s=covered / s)
            return r
        out["clear"] = windows(lambda: keys.fill_(-1), a.reps, a.inner)
        out["raster"] = rate(windows(lambda: fresh(libs["library"]), a.reps, a.inner))
        out["redraw"] = rate(windows(lambda: draw(libs["library"]), a.reps, a.inner))
        d, fc = torch.empty(S, H, W, dtype=torch.float32, device=dev), torch.empty(S, H, W, dtype=torch.int32, device=dev)
        wt = torch.empty(S, H, W, 3, dtype=torch.float64, device=dev)
        on, oc = torch.empty(S, H, W, 3, dtype=torch.float32, device=dev), torch.empty(S, H, W, 3, dtype=torch.float32, device=dev)
        out["resolve"] = rate(windows(lambda: Z.check(libs["library"].vggz_resolve(
            keys, v, V, f, F, n, c, poses, rays, ridx, rays.shape[0], S, H, W, d, fc, wt, on, oc, Z.stream_ptr()), "vggz_resolve"),
            a.reps, a.inner))
        for name, _ in VARIANTS:
            out["raster_" + name] = rate(windows(lambda: fresh(libs[name]), a.reps, a.inner))
            fresh(libs[name])
            assert torch.equal(keys, reference[wname]), f"variant {name} changed the keys"   # the result does not depend on it
        if wname == "mesh":
            vis = torch.empty(S, V, dtype=torch.uint8, device=dev)
            r = windows(lambda: Z.check(libs["library"].vggz_point_visibility(v, V, d, poses, cams, S, H, W, 0.01, vis, Z.stream_ptr()),
                                        "vggz_point_visibility"), a.reps, a.inner)
            r.update(points_per_s=V * S / (r["ms_median"] / 1e3), visible_share=float(vis.float().mean().item()))
            res["visibility"] = r
        for k, r in out.items():
            if isinstance(r, dict):
                print(wname, k, json.dumps(r), flush=True)
                assert math.isfinite(r["ms_median"])
        print(wname, json.dumps({k: r for k, r in out.items() if not isinstance(r, dict)}), flush=True)
    print("visibility", json.dumps(res["visibility"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
