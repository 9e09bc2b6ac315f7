"""GPU times of the registration library (csrc/icp/icp.hip); writes profiles/icp_times.json.  Medians of --reps windows of
--inner calls between device events after a warm-up, min .. max beside (the method of scripts/time_mvs.py); the new code and
its yardstick are timed in ALTERNATING windows of the same call.

Workloads:
  mesh      the mesh vertices of scripts/time_meshing.py (9 depth maps of 512 x 512, 256^3 nodes) against themselves displaced
            by half a voxel, POINT TO POINT, scale estimated, max_dist = cell = 2 voxels.  (That scene is an exact plane and
            its vertex normals are exactly (0, 0, +-1): point to plane is singular on it and the first update would stop with
            "degenerate"; point to point is well posed there, three residual rows per pair.)
  uniform   --points uniform points in the unit cube (one per cell) against themselves displaced by a quarter of a cell, point
            to plane with random unit normals
Per workload:
  fused             vggi_icp_step + vggi_icp_update on a prepared visiting order: one ICP iteration
  step_only         the step kernel alone
  composed          the YARDSTICK: the same iteration from the parent's public API -- sim3.transform_points,
                    PointGrid.nearest, torch gathers and torch sums of the same 38 numbers (no solve: it is not charged)
  composed_prepared the same with the queries' visiting order prepared (the sort taken out): kernel against kernel
  run30             registration.icp, 30 iterations end to end with tolerances that never stop it (the sort, the final step
                    and the read-back included); its status and iteration count are recorded and 30 iterations asserted
  groups            the step + update for other VGGI_GROUPS x VGGI_BLOCK, from variant builds (--build-variants makes them
                    under vggsfm_amd/_variants/ by the library's own Makefile; without them the section is left out)
The fused iteration must have the lower median and its min .. max must not overlap the yardstick's: asserted.
    timeout -k 10 500 python scripts/time_icp.py
"""
import argparse
import ctypes
import json
import os
import platform
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

VARIANTS = ((128, 256), (256, 256), (512, 256), (1024, 256), (2048, 256), (512, 128), (1024, 128), (256, 512))
VARIANT_DIR = os.path.join(ROOT, "vggsfm_amd", "_variants")


def variant_path(groups, block):
    return os.path.join(VARIANT_DIR, f"libvggsfm_amd_icp_g{groups}_b{block}.so")


def build_variants():
    """sidelib.mk's own recipe with the two constants defined: one set of flags"""
    os.makedirs(VARIANT_DIR, exist_ok=True)
    for groups, block in VARIANTS:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "vggsfm_amd", "csrc", "icp"), f"OUT={variant_path(groups, block)}",
                               f"OBJDIR=_obj_g{groups}_b{block}", f"EXTRA=-DVGGI_GROUPS={groups} -DVGGI_BLOCK={block}"])


def alternating(fns, reps, inner):
    """{name: median / min / max ms per call}: per repetition one window of `inner` calls of each function, in turn"""
    import torch
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            ts[name].append(e0.elapsed_time(e1) / inner)
    return {k: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for k, v in ts.items()}


def workload(name, points, normals, shift, cell, a, res, metric):
    import torch
    from vggsfm_amd import _lib, _lib_icp as I, nearest, registration, sim3

    dev = points.device
    target = registration.Target(nearest.PointGrid(points, cell), normals, cell)
    grid = target.grid
    source = (points + shift).contiguous()
    M = source.shape[0]
    r, r2 = cell, cell * cell
    center = registration.default_center(target)
    eye, zero = torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    state0 = registration.make_state(1.0, eye, zero, center, dev)
    state = state0.clone()
    visit = registration._visit(target, source, state)
    work = registration._workspace(dev)
    c = torch.tensor(center, dtype=torch.float64, device=dev)
    s_dev, R_dev, t_dev = state0[2], state0[3:12].reshape(3, 3), state0[12:15]

    def launch(st):
        registration._launch_step(source, visit, target, st, r, r2, metric, True, 0, 0.0, work, None)

    def step():
        launch(state0)

    def fused():
        state.copy_(state0)                                  # the same iteration every time (18 doubles, device to device)
        launch(state)
        registration.check(registration._L.vggi_icp_update(work, state, 1, 6, 0.0, 0.0, 0.0, 0.0, None, 0, registration.stream_ptr()),
                           "vggi_icp_update")

    def composed():
        x = sim3.transform_points(source, s_dev, R_dev, t_dev)
        nn = grid.nearest(x, r)
        ok = nn.index >= 0
        idx = nn.index.clamp(min=0).long()
        y, n = points[idx], normals[idx]
        w = ok.to(torch.float64)
        e, z = x - y, x - c
        if metric == 1:
            res_ = (n * e).sum(1)
            J = torch.cat([torch.linalg.cross(z, n), n, (n * z).sum(1, keepdim=True)], 1)
            sq = res_ * res_
        else:                                                # rows k = 0, 1, 2 of [-[z]x, I, z] per pair, pair-major
            o, i = torch.zeros_like(z[:, 0]), torch.ones_like(z[:, 0])
            J = torch.stack([torch.stack([o, z[:, 2], -z[:, 1], i, o, o, z[:, 0]], 1), torch.stack([-z[:, 2], o, z[:, 0], o, i, o, z[:, 1]], 1),
                             torch.stack([z[:, 1], -z[:, 0], o, o, o, i, z[:, 2]], 1)], 1).reshape(-1, 7)
            res_, sq = e.reshape(-1), (e * e).sum(1)
            w3 = w.repeat_interleave(3)
        wJ = J * (w if metric == 1 else w3)[:, None]
        return wJ.T @ J, wJ.T @ res_, w.sum(), (w * sq).sum(), sq.sum(), ok.sum()

    def composed_prepared():
        grid._visit = lambda q: visit
        try:
            return composed()
        finally:
            del grid._visit
    out = res[name] = {"points": int(M), "cell": cell, "dims": grid.dims}
    out.update(alternating({"fused": fused, "composed": composed, "step_only": step, "composed_prepared": composed_prepared},
                           a.reps, a.inner))
    # the two compute the same system
    fused()
    got = registration._unpack(registration._sums(work).cpu())
    H, g, _, cost, _, count = composed()
    out["pairs"] = got[5]
    assert got[5] == int(count) and abs(got[3] - float(cost)) <= 1e-9 * max(float(cost), 1e-300)
    assert float((got[0] - H.cpu()).abs().max()) <= 1e-9 * float(H.abs().max())
    name_of = {0: "point_to_point", 1: "point_to_plane"}[metric]
    run = lambda: registration.icp(source, target, r, iterations=30, metric=name_of, estimate_scale=True, rotation_tol=-1.0,
                                   translation_tol=-1.0, scale_tol=-1.0)
    out["run30"] = alternating({"icp": run}, a.reps, 2)["icp"]
    reg = run()
    out["run30"].update(status=reg.status, iterations=reg.iterations, rmse=reg.rmse, fitness=reg.fitness)
    assert reg.iterations == 30 and reg.status == "running", f"{name}: the 30-iteration run stopped: {reg.status} after {reg.iterations}"
    # the update timed in `fused` must have done its whole work: one (step, update) leaves the state running, one iteration made
    fused()
    after = state.cpu()
    out["fused_update_status"], out["metric"] = registration.I.STATUS[int(after[0])], name_of
    assert int(after[0]) == 0 and int(after[1]) == 1, f"{name}: the timed update stopped early"
    f, y = out["fused"], out["composed"]
    out["speedup_median"] = y["ms_median"] / f["ms_median"]
    print(name, json.dumps(out), flush=True)
    assert f["ms_median"] < y["ms_median"] and f["ms_max"] < y["ms_min"], f"{name}: the fused iteration does not beat the composed one"
    # other spreads of the same work
    groups = {}
    for G, B in VARIANTS:
        path = variant_path(G, B)
        if not os.path.exists(path):
            continue
        L = ctypes.CDLL(path)
        _lib.bind(L, I.SIGNATURES)
        ws = torch.empty(G * I.WORDS, dtype=torch.float64, device=dev)

        def variant(L=L, ws=ws):
            state.copy_(state0)
            registration.check(L.vggi_icp_step(source, visit, M, grid.points_sorted, grid.order, grid.cell_start, grid.num_points,
                                               *grid._grid_args(), normals, state, r, r2, metric, 1, 0, 0.0, ws, None,
                                               registration.stream_ptr()), "vggi_icp_step")
            registration.check(L.vggi_icp_update(ws, state, 1, 6, 0.0, 0.0, 0.0, 0.0, None, 0, registration.stream_ptr()),
                               "vggi_icp_update")
        groups[f"{G}x{B}"] = variant
    if groups:
        out["groups"] = alternating(groups, a.reps, a.inner)
        print(name, "groups", json.dumps(out["groups"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=9)
    ap.add_argument("--nodes", type=int, default=256)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--build-variants", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_times.json"))
    a = ap.parse_args()
    if a.build_variants:
        build_variants()
        return
    import torch
    from time_fusion import scene
    from vggsfm_amd import _lib_icp as I, meshing
    assert torch.cuda.is_available(), "needs an MI355X"
    prop = torch.cuda.get_device_properties(0)
    res = {"device": torch.cuda.get_device_name(0), "arch": getattr(prop, "gcnArchName", ""), "compute_units": prop.multi_processor_count,
           "memory_gb": round(prop.total_memory / 2 ** 30), "host": platform.node(), "reps": a.reps, "inner": a.inner,
           "groups": I.GROUPS, "block": I.BLOCK}
    dev = torch.device("cuda")
    depth, colors, poses, cams = scene(a.size, a.views)
    side = 4.0 * a.size / (1.25 * a.size)
    voxel = side / (a.nodes - 1)
    vol = meshing.TSDFVolume((-side / 2 + 0.013, -side / 2 + 0.007, 4.0 - side / 2 + 0.011), voxel, (a.nodes,) * 3)
    vol.integrate(depth, poses, cams, None, colors, 4.0 * voxel)
    mesh = vol.extract(1.0)
    del vol, depth, colors
    v = mesh.vertices.to(torch.float64).contiguous()
    nrm = mesh.normals.to(torch.float64).contiguous()
    workload("mesh", v, nrm, torch.tensor([0.3, -0.3, 0.26], dtype=torch.float64, device=dev) * voxel, 2.0 * voxel, a, res, 0)
    g = torch.Generator(device="cuda").manual_seed(1)
    n = a.points
    p = torch.rand(n, 3, generator=g, device=dev, dtype=torch.float64)
    d = torch.randn(n, 3, generator=g, device=dev, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    cell = n ** (-1.0 / 3.0)
    workload("uniform", p, d.contiguous(), torch.tensor([0.15, -0.15, 0.13], dtype=torch.float64, device=dev) * cell, cell, a, res, 1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
