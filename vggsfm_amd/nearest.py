"""The nearest point and the nearest triangle of a large set, for many queries, on the device: a uniform grid built once
and queried by one lane per query, as HIP kernels (csrc/nn/nn.hip); no namesake in the reference.

    PointGrid(points, cell)                  .nearest(queries, max_dist) -> Nearest(index, distance, dist2, count)
    TriangleGrid(vertices, faces, cell)      .nearest(queries, max_dist) -> NearestFace(face, distance, dist2, closest)
    nearest_points / nearest_faces           the two in one call, cell = max_dist
    filter_radius_outliers                   the points of a cloud with too few neighbours within a radius
    distance_stats                           found / below-threshold counts and the sums of d and d^2 over dist2

A result is the lexicographic minimum of (squared distance, index) over the candidates within max_dist and a count of them:
it does not depend on the order of the points, on the traversal or on how the kernel spreads its work, so two runs give the
same bits.  What is torch here is plumbing: allocation, the bounding box, ONE stable sort of int32 cell ids per grid and one
per set of queries, the exclusive sum of the per-face cell counts and the gather of the sorted pairs' face column."""
import math
from collections import namedtuple

import torch

from . import _lib_nn as N
from ._lib_nn import check, require_gpu, stream_ptr

_L = N.lib()          # no fallback: importing the search without its library is an error

Nearest = namedtuple("Nearest", "index distance dist2 count")
NearestFace = namedtuple("NearestFace", "face distance dist2 closest")
Stats = namedtuple("Stats", "num found below sum_d sum_d2")


def _xyz(t, what):
    t = torch.as_tensor(t)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{what} must be (N,3), got {tuple(t.shape)}")
    require_gpu(t)
    return t.to(torch.float64).contiguous()


def _radius(max_dist):
    r = float(max_dist)
    if not r > 0.0:
        raise ValueError(f"max_dist must be > 0, got {max_dist}")
    return r, r * r


def _box(points, cell, origin, dims):
    """origin (3 floats) and dims (3 ints) of a grid: those given, else the box of the finite points"""
    cell = float(cell)
    if not cell > 0.0 or math.isinf(cell):
        raise ValueError(f"cell must be > 0 and finite, got {cell}")
    if (origin is None) != (dims is None):
        raise ValueError("origin and dims are given together or not at all")
    if origin is None:
        ok = torch.isfinite(points).all(dim=1) if points.numel() else torch.zeros(0, dtype=torch.bool)
        if bool(ok.any()):
            lo, hi = points[ok].min(dim=0).values.tolist(), points[ok].max(dim=0).values.tolist()
        else:
            lo, hi = [0.0] * 3, [0.0] * 3
        origin, dims = lo, [int(math.floor((h - l) / cell)) + 1 for l, h in zip(lo, hi)]
    origin, dims = [float(o) for o in origin], [int(d) for d in dims]
    if len(origin) != 3 or len(dims) != 3 or not all(math.isfinite(o) for o in origin):
        raise ValueError(f"origin must be 3 finite numbers and dims 3 integers, got {origin} {dims}")
    if min(dims) < 1:
        raise ValueError(f"every dim must be >= 1, got {dims}")
    if dims[0] * dims[1] * dims[2] > N.MAX_CELLS:
        raise ValueError(f"a grid of {dims} has more than 2^25 cells: choose a larger cell")
    return cell, origin, dims


class _Grid:
    """origin, cell, dims; the cells of points and the visiting order of queries"""

    def _set_box(self, points, cell, origin, dims):
        self.cell, self.origin, self.dims = _box(points, cell, origin, dims)
        self.num_cells = self.dims[0] * self.dims[1] * self.dims[2]

    def _grid_args(self):
        return (*self.origin, self.cell, *self.dims)

    def cells(self, points):
        """(N,) int32 cell ids of points (N,3) by the grid's rule; -1 for a non-finite point"""
        points = _xyz(points, "points")
        out = torch.empty(points.shape[0], dtype=torch.int32, device=points.device)
        check(_L.vggn_point_cells(points, points.shape[0], *self._grid_args(), out, stream_ptr()), "vggn_point_cells")
        return out

    def _cell_start(self, sorted_cell):
        start = torch.empty(self.num_cells + 1, dtype=torch.int32, device=self.device)
        check(_L.vggn_cell_start(sorted_cell, sorted_cell.shape[0], self.num_cells, start, stream_ptr()), "vggn_cell_start")
        return start

    def _visit(self, queries):
        """the order in which the lanes take the queries: that of the queries' own cells, so that a wavefront walks the same
        few cells (measured against the given order in DESIGN.md section 34; the outputs do not depend on it)"""
        return torch.sort(self.cells(queries), stable=True).indices.to(torch.int32)

    def _queries(self, queries):
        queries = _xyz(queries, "queries").to(self.device)
        return queries, self._visit(queries), queries.shape[0]


class PointGrid(_Grid):
    """points (N,3) on a uniform grid of `cell`-sized cells over origin (3) and dims (3) (default: the box of the finite
    points).  A point outside the box lives in the border cell; a non-finite point takes part in nothing.  Attributes:
    points_sorted (N,3) and order (N,) int32 -- the points in the stable order of their cells and their original indices --
    and cell_start (C + 1,) int32."""

    def __init__(self, points, cell, origin=None, dims=None):
        points = _xyz(points, "points")
        self.device = points.device
        self._set_box(points, cell, origin, dims)
        self.num_points = n = points.shape[0]
        cells, perm = torch.sort(self.cells(points), stable=True)
        self.order = perm.to(torch.int32)
        self.points_sorted = torch.empty(n, 3, dtype=torch.float64, device=self.device)
        check(_L.vggn_gather_points(points, self.order, n, self.points_sorted, stream_ptr()), "vggn_gather_points")
        self.cell_start = self._cell_start(cells)

    def nearest(self, queries, max_dist, exclude_self=False):
        """queries (M,3) -> Nearest(index (M,) int32, -1 = none; distance, dist2 (M,) float64, +inf = none; count (M,) int32,
        the number of grid points within max_dist).  exclude_self: the grid point whose index equals the query's is left out
        (a cloud against itself)."""
        r, r2 = _radius(max_dist)
        queries, visit, M = self._queries(queries)
        index = torch.empty(M, dtype=torch.int32, device=self.device)
        dist2 = torch.empty(M, dtype=torch.float64, device=self.device)
        count = torch.empty(M, dtype=torch.int32, device=self.device)
        check(_L.vggn_nearest_point(self.points_sorted, self.order, self.cell_start, self.num_points, *self._grid_args(), queries,
                                    visit, M, r, r2, int(bool(exclude_self)), index, dist2, count, stream_ptr()),
              "vggn_nearest_point")
        return Nearest(index, torch.sqrt(dist2), dist2, count)


def _mesh_tensors(mesh_or_vertices, faces):
    if faces is None:
        mesh_or_vertices, faces = mesh_or_vertices.vertices, mesh_or_vertices.faces
    vertices, faces = _xyz(mesh_or_vertices, "vertices"), torch.as_tensor(faces)
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"faces must be (F,3) int32, got {tuple(faces.shape)} {faces.dtype}")
    return vertices, faces.contiguous().to(vertices.device)


class TriangleGrid(_Grid):
    """A triangle mesh -- a meshing.Mesh, or vertices (V,3) and faces (F,3) int32 -- on a uniform grid: every valid face is
    registered in each cell its axis-aligned box reaches (default box: that of the finite vertices).  A face with a row
    outside [0, V), two equal rows, a non-finite vertex or no area is skipped.  Attributes: cell_faces (P,) int32, the faces
    in the stable order of their cells, and cell_start (C + 1,) int32."""

    def __init__(self, vertices, faces=None, cell=None, origin=None, dims=None):
        if cell is None and isinstance(faces, (int, float)):          # TriangleGrid(mesh, cell)
            faces, cell = None, faces
        if cell is None:
            raise ValueError("a TriangleGrid needs a cell size")
        self.vertices, self.faces = _mesh_tensors(vertices, faces)
        self.device = dev = self.vertices.device
        self._set_box(self.vertices, cell, origin, dims)
        V, F = self.vertices.shape[0], self.faces.shape[0]
        counts = torch.zeros(F, dtype=torch.int32, device=dev)
        check(_L.vggn_face_cell_counts(self.vertices, V, self.faces, F, *self._grid_args(), counts, stream_ptr()),
              "vggn_face_cell_counts")
        ends = torch.cumsum(counts, 0, dtype=torch.int64)
        self.num_pairs = P = int(ends[-1]) if F else 0
        if P > N.MAX_PAIRS:
            raise ValueError(f"the faces reach {P} cells in all, more than 2^31 - 1 (cell, face) pairs: choose a larger cell")
        pair_cell = torch.empty(P, dtype=torch.int32, device=dev)
        pair_face = torch.empty(P, dtype=torch.int32, device=dev)
        check(_L.vggn_face_cell_pairs(self.vertices, V, self.faces, F, *self._grid_args(), ends - counts, P, pair_cell, pair_face,
                                      stream_ptr()), "vggn_face_cell_pairs")
        cells, perm = torch.sort(pair_cell, stable=True)
        self.cell_faces = pair_face[perm].contiguous()
        self.cell_start = self._cell_start(cells)

    def nearest(self, queries, max_dist, return_closest=False):
        """queries (M,3) -> NearestFace(face (M,) int32, -1 = none; distance, dist2 (M,) float64, +inf = none; closest (M,3)
        float64, the nearest point of that face, NaN = none -- or None)."""
        r, r2 = _radius(max_dist)
        queries, visit, M = self._queries(queries)
        face = torch.empty(M, dtype=torch.int32, device=self.device)
        dist2 = torch.empty(M, dtype=torch.float64, device=self.device)
        closest = torch.empty(M, 3, dtype=torch.float64, device=self.device) if return_closest else None
        check(_L.vggn_nearest_face(self.vertices, self.vertices.shape[0], self.faces, self.faces.shape[0], self.cell_faces,
                                   self.cell_start, self.num_pairs, *self._grid_args(), queries, visit, M, r, r2, face, dist2,
                                   closest, stream_ptr()), "vggn_nearest_face")
        return NearestFace(face, torch.sqrt(dist2), dist2, closest)


def nearest_points(points, queries, max_dist, cell=None, exclude_self=False):
    """The nearest of points (N,3) to each of queries (M,3) within max_dist -> Nearest.  cell: the grid's (default max_dist)."""
    r, _ = _radius(max_dist)
    return PointGrid(points, r if cell is None else cell).nearest(queries, r, exclude_self)


def nearest_faces(mesh, queries, max_dist, cell=None, return_closest=False):
    """The nearest face of a meshing.Mesh (or a (vertices, faces) pair) to each of queries (M,3) within max_dist ->
    NearestFace."""
    r, _ = _radius(max_dist)
    vertices, faces = mesh if isinstance(mesh, (tuple, list)) and len(mesh) == 2 else (mesh, None)
    return TriangleGrid(vertices, faces, r if cell is None else cell).nearest(queries, r, return_closest)


def filter_radius_outliers(cloud_or_xyz, radius, min_neighbors):
    """Radius outlier removal: keep the points with at least min_neighbors OTHER points within `radius`.  Given points (N,3)
    -> the (N,) bool keep-mask; given a fusion.FusedCloud -> (mask, the cloud with every field filtered)."""
    cloud = cloud_or_xyz if hasattr(cloud_or_xyz, "_fields") and "xyz" in cloud_or_xyz._fields else None
    xyz = _xyz(cloud.xyz if cloud is not None else cloud_or_xyz, "points")
    keep = PointGrid(xyz, radius).nearest(xyz, radius, exclude_self=True).count >= int(min_neighbors)
    if cloud is None:
        return keep
    return keep, type(cloud)(*(None if f is None else f[keep] for f in cloud))


def distance_stats(dist2, thresholds=()):
    """dist2 (M,) float64 squared distances (+inf = none) -> Stats(num = M, found = #finite, below = [#{sqrt(d2) < tau}] per
    threshold (at most 8), sum_d, sum_d2 = the sums of sqrt(d2) and d2 over the found) as Python numbers.  The counts are exact
    and the sums are taken in a fixed order: two runs give the same bits."""
    dist2 = torch.as_tensor(dist2)
    if dist2.dim() != 1 or dist2.dtype != torch.float64:
        raise ValueError(f"dist2 must be (M,) float64, got {tuple(dist2.shape)} {dist2.dtype}")
    require_gpu(dist2)
    dist2 = dist2.contiguous()
    taus = [float(t) for t in thresholds]
    if len(taus) > N.MAX_THRESHOLDS:
        raise ValueError(f"at most {N.MAX_THRESHOLDS} thresholds to a call, got {len(taus)}")
    K, dev = len(taus), dist2.device
    host = torch.tensor(taus, dtype=torch.float64) if K else None
    counts = torch.empty(1 + K, dtype=torch.int64, device=dev)
    sums = torch.empty(2, dtype=torch.float64, device=dev)
    work = torch.empty(N.STATS_GROUPS * N.STATS_WORDS, dtype=torch.float64, device=dev)
    check(_L.vggn_distance_stats(dist2, dist2.shape[0], host, K, counts, sums, work, stream_ptr()), "vggn_distance_stats")
    counts, sums = counts.tolist(), sums.tolist()
    return Stats(dist2.shape[0], counts[0], counts[1:], sums[0], sums[1])
