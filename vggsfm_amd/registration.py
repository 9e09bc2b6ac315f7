"""Registration of a dense model to a reference by ICP on the device (csrc/icp/icp.hip); no namesake
in the reference.  Convention of vggsfm_amd.sim3: ``target ~ scale * R @ source + t``.

    estimate_normals(points, radius)            -> Normals(normal, curvature, count): PCA over the neighbours within a radius
    make_target(reference, cell)                -> Target: a point set, a fusion.FusedCloud or a meshing.Mesh on a grid
    icp_step(source, target, transform, ...)    -> Step(H, g, cost, weight, sq_error, count, index): the normal equations
    icp(source, target, max_dist, ...)          -> Registration(scale, R, t, status, iterations, history, rmse, fitness)

One iteration is two launches: the fused step (transform a source point, walk the target's grid to its nearest point or
triangle, form the residual and its Jacobian row, accumulate the normal equations -- no correspondence is stored) and the
update (solve, compose, test for convergence) of a transform that stays on the device.  The sums are taken in a fixed order:
two runs give the same bits.  What torch does here is plumbing, per stage of a run: allocation, the 18 doubles of the start
state copied to the device, the sort of the visiting order (once for the iterations, once more for the sums at the final
transform, which run on a clone of the state with its status reset), one concatenation and ONE read-back (a stage that
stops early on "too few" or "degenerate" before the last costs a second)."""
import math
from collections import namedtuple

import torch

from . import _lib_icp as I
from . import nearest, sim3
from ._lib_icp import check, require_gpu, stream_ptr

_L = I.lib()          # no fallback: importing the registration without its library is an error

Normals = namedtuple("Normals", "normal curvature count")
Target = namedtuple("Target", "grid normals cell")
Step = namedtuple("Step", "H g cost weight sq_error count index")
Registration = namedtuple("Registration", "scale R t status iterations history rmse fitness")

METRICS = {"point_to_point": 0, "point_to_plane": 1}
LOSSES = {None: 0, "huber": 1, "tukey": 2}
HISTORY_FIELDS = ("count", "weight", "cost", "sq_error", "rotation", "translation", "scale_step")


def _is_mesh(x):
    return hasattr(x, "_fields") and "faces" in x._fields


def estimate_normals(points, radius, min_neighbors=5, toward=None, cell=None):
    """Normals of points (N,3) (or of a nearest.PointGrid) from the covariance of the neighbours within `radius`: the unit
    eigenvector of the smallest eigenvalue, turned towards the viewpoint `toward` (3 numbers) or else so that its first
    non-zero component is positive; curvature = l0 / (l0 + l1 + l2); count = the neighbours (the point itself among them).
    Below min_neighbors the normal is NaN."""
    r, r2 = nearest._radius(radius)
    grid = points if isinstance(points, nearest.PointGrid) else nearest.PointGrid(points, r if cell is None else cell)
    if int(min_neighbors) < 1:
        raise ValueError(f"min_neighbors must be >= 1, got {min_neighbors}")
    n, dev = grid.num_points, grid.device
    host = None
    if toward is not None:
        host = torch.as_tensor(toward, dtype=torch.float64).reshape(-1).cpu().contiguous()
        if host.numel() != 3 or not bool(torch.isfinite(host).all()):
            raise ValueError("toward must be 3 finite numbers")
    normal = torch.empty(n, 3, dtype=torch.float64, device=dev)
    curvature = torch.empty(n, dtype=torch.float64, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    check(_L.vggi_radius_normals(grid.points_sorted, grid.order, grid.cell_start, n, *grid._grid_args(), r, r2, int(min_neighbors),
                                 host, normal, curvature, count, stream_ptr()), "vggi_radius_normals")
    return Normals(normal, curvature, count)


def make_target(reference, cell, normal_radius=None, min_neighbors=5):
    """What a source is registered to: `reference` -- points (N,3), a fusion.FusedCloud (its normals are taken) or a
    meshing.Mesh (a nearest.TriangleGrid: the faces' own normals) -- on a grid of `cell`-sized cells.  normal_radius: estimate
    the normals of a point set that has none (estimate_normals); without them only point-to-point is possible."""
    if isinstance(reference, Target):
        return reference if reference.cell == float(cell) else make_target(_reference_of(reference), cell)
    if _is_mesh(reference):
        return Target(nearest.TriangleGrid(reference.vertices, reference.faces, cell), None, float(cell))
    cloud = hasattr(reference, "_fields") and "xyz" in reference._fields
    grid = nearest.PointGrid(reference.xyz if cloud else reference, cell)
    normals = None
    if cloud and reference.normal is not None:
        normals = reference.normal.to(device=grid.device, dtype=torch.float64).contiguous()
    elif normal_radius is not None:
        normals = estimate_normals(grid, normal_radius, min_neighbors).normal
    return Target(grid, normals, float(cell))


def _reference_of(target):
    """the reference a Target was made of, for a rebuild at another cell (the normals travel with it)"""
    grid = target.grid
    if isinstance(grid, nearest.TriangleGrid):
        return namedtuple("Mesh", "vertices faces")(grid.vertices, grid.faces)
    points = torch.empty_like(grid.points_sorted)
    points[grid.order.long()] = grid.points_sorted
    if target.normals is None:
        return points
    return namedtuple("Cloud", "xyz normal")(points, target.normals)


def default_center(target):
    """the centre of the target grid's box: host numbers"""
    g = target.grid
    return [o + 0.5 * d * g.cell for o, d in zip(g.origin, g.dims)]


def _source(source, device):
    source = source.xyz if hasattr(source, "_fields") and "xyz" in source._fields else (source.vertices if _is_mesh(source) else source)
    return nearest._xyz(source, "source").to(device)


def _options(target, metric, loss, loss_scale):
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {sorted(METRICS)}, got {metric!r}")
    if loss not in LOSSES:
        raise ValueError(f"loss must be None, 'huber' or 'tukey', got {loss!r}")
    if LOSSES[loss] and not (loss_scale is not None and float(loss_scale) > 0.0):
        raise ValueError(f"loss {loss!r} needs loss_scale > 0, got {loss_scale}")
    if METRICS[metric] == 1 and isinstance(target.grid, nearest.PointGrid) and target.normals is None:
        raise ValueError("point_to_plane needs target normals: a FusedCloud, a Mesh, or make_target(..., normal_radius=)")
    return METRICS[metric], LOSSES[loss], float(loss_scale) if LOSSES[loss] else 0.0


def make_state(scale, R, t, center, device):
    """(VGGI_STATE_WORDS,) float64 on the device: status running, 0 iterations, the transform and the centre"""
    R = torch.as_tensor(R, dtype=torch.float64).reshape(9).cpu()
    t = torch.as_tensor(t, dtype=torch.float64).reshape(3).cpu()
    c = torch.as_tensor(center, dtype=torch.float64).reshape(3).cpu()
    host = torch.cat([torch.tensor([0.0, 0.0, float(scale)], dtype=torch.float64), R, t, c])
    if not bool(torch.isfinite(host).all()):
        raise ValueError("the transform and the centre must be finite")
    return host.to(device)


def _launch_step(source, visit, target, state, r, r2, metric, estimate_scale, loss, loss_scale, work, out_index):
    g = target.grid
    M = source.shape[0]
    if isinstance(g, nearest.TriangleGrid):
        check(_L.vggi_icp_step_mesh(source, visit, M, g.vertices, g.vertices.shape[0], g.faces, g.faces.shape[0], g.cell_faces,
                                    g.cell_start, g.num_pairs, *g._grid_args(), state, r, r2, metric, int(estimate_scale), loss,
                                    loss_scale, work, out_index, stream_ptr()), "vggi_icp_step_mesh")
    else:
        check(_L.vggi_icp_step(source, visit, M, g.points_sorted, g.order, g.cell_start, g.num_points, *g._grid_args(),
                               target.normals, state, r, r2, metric, int(estimate_scale), loss, loss_scale, work, out_index,
                               stream_ptr()), "vggi_icp_step")


def _visit(target, source, state):
    """the order of the source points' cells at the state's transform (no host work)"""
    moved = sim3.transform_points(source, state[2], state[3:12].reshape(3, 3), state[12:15])
    return target.grid._visit(moved)


def _workspace(device):
    return torch.empty(I.GROUPS * I.WORDS, dtype=torch.float64, device=device)


def _sums(work):
    out = torch.empty(I.WORDS, dtype=torch.float64, device=work.device)
    check(_L.vggi_icp_sums(work, out, stream_ptr()), "vggi_icp_sums")
    return out


def _unpack(sums):
    """(WORDS,) host float64 -> H (7,7), g (7,), weight, cost, sq_error, count"""
    H = torch.zeros(7, 7, dtype=torch.float64)
    iu = torch.triu_indices(7, 7)
    H[iu[0], iu[1]] = sums[:28]
    H = H + H.triu(1).T
    count = int(sums[38:39].view(torch.int64)[0])
    return H, sums[28:35].clone(), float(sums[35]), float(sums[36]), float(sums[37]), count


def icp_step(source, target, transform=None, max_dist=None, metric="point_to_plane", estimate_scale=False, loss=None,
             loss_scale=None, center=None, return_index=False, visit=None):
    """The normal equations of one ICP iteration at `transform` = (scale, R, t) (default: the identity): Step(H (7,7) and
    g (7,) over (omega, tau, lambda) about `center` (default: the centre of the target's box) -- the lambda row is zero
    without estimate_scale --, cost = sum w r^2, weight = sum w, sq_error = sum r^2, count, index (M,) int32 of the pairs
    (-1 = none) with return_index) as host tensors and Python numbers."""
    if max_dist is None:
        raise ValueError("icp_step needs max_dist")
    r, r2 = nearest._radius(max_dist)
    m, l, k = _options(target, metric, loss, loss_scale)
    source = _source(source, target.grid.device)
    scale, R, t = transform if transform is not None else (1.0, torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64))
    state = make_state(scale, R, t, default_center(target) if center is None else center, source.device)
    visit = _visit(target, source, state) if visit is None else visit.to(device=source.device, dtype=torch.int32).contiguous()
    work = _workspace(source.device)
    # (-1 where no lane writes: a caller's visit order that leaves a point out)
    index = torch.full((source.shape[0],), -1, dtype=torch.int32, device=source.device) if return_index else None
    _launch_step(source, visit, target, state, r, r2, m, estimate_scale, l, k, work, index)
    H, g, weight, cost, sq_error, count = _unpack(_sums(work).cpu())
    return Step(H, g, cost, weight, sq_error, count, index)


def icp(source, target, max_dist, init=None, iterations=30, metric="point_to_plane", estimate_scale=False, loss=None,
        loss_scale=None, rotation_tol=1e-9, translation_tol=1e-9, scale_tol=1e-9, min_correspondences=6, damping=0.0,
        resort_every=0, center=None, cell=None):
    """Register `source` (points (M,3), a FusedCloud or a Mesh's vertices) to `target` (make_target's, or a reference it is
    made of with cell = the first max_dist).  max_dist: a number or a sequence of stages, coarse to fine, each of at most
    `iterations` iterations; the grid is rebuilt when its cell (= the stage's max_dist unless `cell` is given) changes.
    init: (scale, R, t).  A stage ends when every increment is below its tolerance ("converged"), when fewer than
    min_correspondences pairs are left ("too few"), when the normal equations are singular ("degenerate") or after
    `iterations` ("running").  damping: mu of a Levenberg step, the diagonal times 1 + mu.  resort_every: recompute the
    visiting order every so many iterations (it is computed once per stage otherwise; it moves time and the last bits of
    the sums, nothing else).

    Returns Registration(scale, R (3,3), t (3,) as host tensors, status, iterations, history -- a list of dicts per iteration
    (HISTORY_FIELDS: the sums AT the transform the iteration started from, and the norms of its increment) --, rmse and
    fitness = count / M at the final transform)."""
    stages = [float(s) for s in (max_dist if isinstance(max_dist, (list, tuple)) else [max_dist])]
    if not stages:
        raise ValueError("max_dist is empty")
    iterations = int(iterations)
    if iterations < 1:
        raise ValueError(f"iterations must be >= 1, got {iterations}")
    if int(min_correspondences) < 1 or not float(damping) >= 0.0:
        raise ValueError("min_correspondences must be >= 1 and damping >= 0")
    if not isinstance(target, Target):
        target = make_target(target, stages[0] if cell is None else cell)
    dev = target.grid.device
    source = _source(source, dev)
    m, l, k = _options(target, metric, loss, loss_scale)
    scale, R, t = init if init is not None else (1.0, torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64))
    scale, R, t = float(scale), torch.as_tensor(R).detach().cpu().double(), torch.as_tensor(t).detach().cpu().double()
    history, total, status = [], 0, 0
    work = _workspace(dev)
    for stage, dist in enumerate(stages):
        r, r2 = nearest._radius(dist)
        want = float(dist if cell is None else cell)
        if target.cell != want:
            target = make_target(target, want)
        state = make_state(scale, R, t, default_center(target) if center is None else center, dev)
        rows = torch.zeros(iterations, I.HISTORY_WORDS, dtype=torch.float64, device=dev)
        visit = _visit(target, source, state)

        def _final_sums(state):
            final = state.clone()
            final[0] = 0.0
            _launch_step(source, _visit(target, source, final), target, final, r, r2, m, estimate_scale, l, k, work, None)
            return _sums(work)
        for it in range(iterations):
            if resort_every and it and it % int(resort_every) == 0:
                visit = _visit(target, source, state)
            _launch_step(source, visit, target, state, r, r2, m, estimate_scale, l, k, work, None)
            check(_L.vggi_icp_update(work, state, int(estimate_scale), int(min_correspondences), float(damping), float(rotation_tol),
                                     float(translation_tol), float(scale_tol), rows, iterations, stream_ptr()), "vggi_icp_update")
        last = stage == len(stages) - 1
        parts = [state, rows.reshape(-1)]
        if last:                                  # the sums at the final transform, in the same read-back
            parts.append(_final_sums(state))
        back = torch.cat(parts).cpu()
        status, done = int(back[0]), int(back[1])
        scale, R, t = float(back[2]), back[3:12].reshape(3, 3).clone(), back[12:15].clone()
        hist = back[I.STATE_WORDS:I.STATE_WORDS + iterations * I.HISTORY_WORDS].reshape(iterations, I.HISTORY_WORDS)
        for row in hist[:done].tolist():
            entry = dict(zip(HISTORY_FIELDS, row))
            entry["count"], entry["stage"] = int(entry["count"]), stage
            history.append(entry)
        total += done
        if status in (2, 3) and not last:         # a stage that lost its pairs or its rank ends the run: one more read-back
            back = _final_sums(state).cpu()
            break
    _, _, _, _, sq_error, count = _unpack(back[-I.WORDS:])
    M = source.shape[0]
    rmse = math.sqrt(sq_error / count) if count else math.nan
    return Registration(scale, R, t, I.STATUS[status], total, history, rmse, count / M if M else 0.0)
