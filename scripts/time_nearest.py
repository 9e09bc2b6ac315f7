"""GPU times of the nearest-neighbour library (csrc/nn/nn.hip); writes profiles/nearest_times.json.  Medians of --reps
windows of --inner calls between device events after a warm-up, min .. max beside (the method of scripts/time_mvs.py).

Workloads:
  mesh      the mesh of scripts/time_meshing.py (9 depth maps of 512 x 512 integrated into 256^3 nodes and extracted) against
            its own vertices at max_dist = cell = 2 voxels: the triangle grid's build and query, the point grid's build and
            query (the vertices against themselves, exclude_self) and the statistics of the result
  uniform   --points uniform points in the unit cube against as many uniform queries, the cell such that a cell holds one
            point on average, at max_dist = 1 and 2 cells
Each query is timed in BOTH visiting orders -- "cell" (the queries in the order of their own cells: what the library's
callers get; the time includes computing and sorting the queries' cells) and "given" (the same kernel, the queries as they
come: the grid's _visit replaced by the identity) -- and `kernel_only` times the kernel alone on a visiting order computed
before.  The outputs of the two orders are
asserted equal.  The wavefront-per-cell variant that stages a neighbourhood in LDS was not built.
  cdist     the YARDSTICK, named as such: torch.cdist + min over --yard x --yard points, in chunks of 4096 queries, on the
            same device; its indices must agree with the library's wherever its two nearest distances differ.
No thresholds: the numbers are reported; the parent commit has nothing that does this work.  Run under its own time limit:
    timeout -k 10 500 python scripts/time_nearest.py
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


def time_queries(grid, queries, max_dist, reps, inner, **kw):
    """both visiting orders of grid.nearest, the kernel alone on a prepared order, and the equality of the outputs"""
    import torch
    out = {}
    results = {}
    given = torch.arange(queries.shape[0], dtype=torch.int32, device=queries.device)
    by_cell = grid._visit(queries)
    for order, visit in (("cell", None), ("given", lambda q: given), ("kernel_only_cell", lambda q: by_cell),
                         ("kernel_only_given", lambda q: given.clone())):
        if visit is not None:
            grid._visit = visit                          # in place of the method: a prepared order costs nothing per call
        out[order] = windows(lambda: grid.nearest(queries, max_dist, **kw), reps, inner)
        results[order] = grid.nearest(queries, max_dist, **kw)
        if visit is not None:
            del grid._visit
    for a, b in zip(results["cell"], results["given"]):
        assert (a is None and b is None) or torch.equal(a, b), "the visiting order changed an output"
    first = results["cell"]
    found = int(torch.isfinite(first.dist2).sum().item())
    out.update(queries=int(queries.shape[0]), found=found, queries_per_s_cell=queries.shape[0] / (out["cell"]["ms_median"] / 1e3))
    return out, first


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=9)
    ap.add_argument("--nodes", type=int, default=256)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--yard", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_times.json"))
    a = ap.parse_args()
    import torch
    from vggsfm_amd import meshing, nearest
    assert torch.cuda.is_available(), "needs an MI355X"
    prop = torch.cuda.get_device_properties(0)
    res = {"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "memory_gb": round(prop.total_memory / 2 ** 30), "host": platform.node(), "reps": a.reps, "inner": a.inner}
    dev = torch.device("cuda")

    # ---- the mesh of scripts/time_meshing.py against its own vertices
    depth, colors, poses, cams = scene(a.size, a.views)
    side = 4.0 * a.size / (1.25 * a.size)
    voxel = side / (a.nodes - 1)
    vol = meshing.TSDFVolume((-side / 2 + 0.013, -side / 2 + 0.007, 4.0 - side / 2 + 0.011), voxel, (a.nodes,) * 3)
    vol.integrate(depth, poses, cams, None, colors, 4.0 * voxel)
    mesh = vol.extract(1.0)
    del vol, depth, colors
    v, f = mesh.vertices.contiguous(), mesh.faces.contiguous()
    r = 2.0 * voxel
    out = res["mesh"] = {"vertices": int(v.shape[0]), "faces": int(f.shape[0]), "voxel": voxel, "max_dist": r, "cell": r}
    out["triangle_grid_build"] = windows(lambda: nearest.TriangleGrid(v, f, r), a.reps, a.inner)
    tg = nearest.TriangleGrid(v, f, r)
    out.update(dims=tg.dims, pairs=tg.num_pairs)
    out["nearest_face"], faces = time_queries(tg, v, r, a.reps, a.inner)
    assert float(faces.distance.median().item()) == 0.0, "the vertices are not on their own mesh"
    out["point_grid_build"] = windows(lambda: nearest.PointGrid(v, r), a.reps, a.inner)
    pg = nearest.PointGrid(v, r)
    out["nearest_point_self"], pts = time_queries(pg, v, r, a.reps, a.inner, exclude_self=True)
    out["mean_neighbours"] = float(pts.count.double().mean().item())
    out["distance_stats"] = windows(lambda: nearest.distance_stats(pts.dist2, [voxel, 2 * voxel]), a.reps, a.inner)
    for k, t in out.items():
        print("mesh", k, json.dumps(t), flush=True)

    # ---- uniform points
    g = torch.Generator(device="cuda").manual_seed(1)
    n = a.points
    p, q = torch.rand(n, 3, generator=g, device=dev, dtype=torch.float64), torch.rand(n, 3, generator=g, device=dev, dtype=torch.float64)
    cell = n ** (-1.0 / 3.0)
    out = res["uniform"] = {"points": n, "queries": n, "cell": cell}
    out["point_grid_build"] = windows(lambda: nearest.PointGrid(p, cell), a.reps, a.inner)
    ug = nearest.PointGrid(p, cell)
    out["dims"] = ug.dims
    for cells in (1.0, 2.0):
        key = f"nearest_point_{int(cells)}_cell"
        out[key], got = time_queries(ug, q, cells * cell, a.reps, max(a.inner // 4, 2))
        out[key]["mean_neighbours"] = float(got.count.double().mean().item())
        print("uniform", key, json.dumps(out[key]), flush=True)

    # ---- the yardstick: torch.cdist + min, chunked
    y = a.yard
    py, qy = p[:y].contiguous(), q[:y].contiguous()

    def yardstick(two=False):
        best, arg = [], []
        for s in range(0, y, 4096):
            d = torch.cdist(qy[s:s + 4096], py)
            m = d.topk(2, dim=1, largest=False) if two else d.min(dim=1)
            best.append(m.values)
            arg.append(m.indices)
        return torch.cat(best), torch.cat(arg)
    out = res["cdist_yardstick"] = {"points": y, "queries": y, "what": "torch.cdist + min in chunks of 4096 queries: a yardstick, not a rival"}
    out["cdist_min"] = windows(yardstick, a.reps, 2)
    big = 4.0 * y ** (-1.0 / 3.0)
    out["library_build_and_query"] = windows(lambda: nearest.nearest_points(py, qy, big, cell=big / 2), a.reps, a.inner)
    mine = nearest.nearest_points(py, qy, big, cell=big / 2)
    # cdist forms |a|^2 + |b|^2 - 2 a.b: its distances carry an absolute error near 1e-8 on unit-cube coordinates, so its two
    # nearest count as different only when they are 1e-6 apart
    d, i = yardstick(two=True)
    distinct = (d[:, 1] - d[:, 0]) > 1e-6
    d, i = d[:, 0], i[:, 0]
    inside = mine.index >= 0
    agree = (mine.index.long() == i) | ~distinct | ~inside
    out.update(found=int(inside.sum().item()), index_agreement=bool(agree.all().item()),
               max_distance_difference=float((mine.distance[inside] - d[inside]).abs().max().item()))
    assert out["index_agreement"], "the yardstick names another nearest point"
    print("cdist", json.dumps(out), flush=True)
    for group in res.values():
        if isinstance(group, dict):
            for t in group.values():
                assert not isinstance(t, dict) or "ms_median" not in t or math.isfinite(t["ms_median"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
