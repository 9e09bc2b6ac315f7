"""GPU times of the meshing entries (csrc/tsdf/tsdf.hip); writes profiles/meshing_times.json.  Medians of --reps windows of
--inner calls between device events after a warm-up, min .. max beside (the method of scripts/time_mvs.py):
  integrate     vggv_integrate: 9 views of 512 x 512 (weights 1, colours) into 256^3 nodes, one launch
  count         vggv_mesh_count on that volume: the per-node pass and the scan of the 65 536 groups' counts (two launches)
  emit          vggv_mesh_emit on that volume, outputs pre-allocated
  extract       TSDFVolume.extract: both entries with their allocations and the one host read between them
The scene: cameras on a line in front of a fronto-parallel plane at depth 4 (scripts/time_fusion.py); the grid is a cube
around the part of the plane the middle camera sees.  Beside each time: nodes per second and the bytes the pass must move at
least (every array it reads or writes once), as a share of 8 TB/s of HBM bandwidth -- orientation only.  No thresholds: the
numbers are reported; the parent commit has nothing to compare with.  Run under its own time limit, e.g.
    timeout -k 10 300 python scripts/time_meshing.py
"""
import argparse
import json
import math
import os
import platform
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_fusion import scene  # noqa: E402
from time_mvs import windows  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=9)
    ap.add_argument("--nodes", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshing_times.json"))
    a = ap.parse_args()
    import torch
    from vggsfm_amd import _lib_tsdf as T
    from vggsfm_amd import meshing
    assert torch.cuda.is_available(), "needs an MI355X"
    prop = torch.cuda.get_device_properties(0)
    res = {"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "memory_gb": round(prop.total_memory / 2 ** 30), "host": platform.node(), "reps": a.reps, "inner": a.inner, "size": a.size,
           "views": a.views, "nodes_per_side": a.nodes, "hbm_bytes_per_s_assumed": HBM_BYTES_PER_S}
    L = T.lib()
    depth, colors, poses, cams = scene(a.size, a.views)
    side = 4.0 * a.size / (1.25 * a.size)                                    # what the middle camera sees of the plane z = 4
    voxel = side / (a.nodes - 1)
    origin = (-side / 2 + 0.013, -side / 2 + 0.007, 4.0 - side / 2 + 0.011)
    dims = (a.nodes,) * 3
    N = a.nodes ** 3
    trunc = 4.0 * voxel
    vol = meshing.TSDFVolume(origin, voxel, dims)

    def rate(r, nbytes):
        s = r["ms_median"] / 1e3
        r.update(nodes_per_s=N / s, bytes_min=nbytes, share_of_hbm=nbytes / s / HBM_BYTES_PER_S)
        return r

    def integrate():
        T.check(L.vggv_integrate(depth, None, colors, poses, cams, a.views, a.size, a.size, *origin, voxel, *dims, trunc, vol.tsdf_sum,
                                 vol.weight_sum, vol.rgb_sum, T.stream_ptr()), "vggv_integrate")
    # (every call adds the views again: the sums grow, the work does not change)
    res["integrate"] = rate(windows(integrate, a.reps, a.inner), N * 5 * 8 * 2 + a.views * a.size * a.size * 4 * 4)
    for t in (vol.tsdf_sum, vol.weight_sum, vol.rgb_sum):
        t.zero_()
    integrate()
    count = vol.count(1.0)
    V, F = (int(c) for c in count["counts"].tolist())

    def count_only():
        T.check(L.vggv_mesh_count(vol.tsdf_sum, vol.weight_sum, *dims, 1.0, count["edge_mask"], count["vertex_offset"],
                                  count["face_offset"], count["group_counts"], count["group_offsets"], count["counts"],
                                  T.stream_ptr()), "vggv_mesh_count")
    res["count"] = rate(windows(count_only, a.reps, a.inner), N * (16 + 9))
    dev = depth.device
    out = [torch.empty(max(V, 1), 3, dtype=torch.float64, device=dev), torch.empty(max(V, 1), 3, dtype=torch.float32, device=dev),
           torch.empty(max(V, 1), 3, dtype=torch.float32, device=dev), torch.empty(max(F, 1), 3, dtype=torch.int32, device=dev)]

    def emit_only():
        T.check(L.vggv_mesh_emit(vol.tsdf_sum, vol.weight_sum, vol.rgb_sum, *origin, voxel, *dims, 1.0, count["edge_mask"],
                                 count["vertex_offset"], count["face_offset"], count["group_offsets"], V, F, *out, T.stream_ptr()),
                "vggv_mesh_emit")
    res["emit"] = rate(windows(emit_only, a.reps, a.inner), N * (16 + 9) + V * 48 + F * 12)
    res["extract"] = rate(windows(lambda: vol.extract(1.0), a.reps, max(1, a.inner // 4)), 2 * N * (16 + 9) + V * 48 + F * 12)
    res.update(vertices=V, faces=F, valid_nodes=int((vol.weight_sum >= 1.0).sum()))
    for k in ("integrate", "count", "emit", "extract"):
        print(k, json.dumps(res[k]), flush=True)
        assert math.isfinite(res[k]["ms_median"])
    print(json.dumps({k: res[k] for k in ("vertices", "faces", "valid_nodes")}))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
