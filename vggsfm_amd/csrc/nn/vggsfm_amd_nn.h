/*
 * vggsfm_amd -- the nearest point and the nearest triangle of a large set, for many queries, on a uniform grid; and the
 * counts and sums over such distances that accuracy, completeness and F-score are made of (libvggsfm_amd_nn.so, a library of
 * its own: the entries of the other libraries and the headers under include/ are closed, counted sets).
 *
 * Conventions of include/vggsfm_amd.h hold: device pointers, `stream` a hipStream_t as void*, asynchronous (no entry
 * synchronises with the host), no allocation, VGG_OK (0) or a negative VGG_ERR_* code.  The names carry the prefix vggn_;
 * their rows stand in vggsfm_amd/_lib_nn.py.  One argument is a HOST array: thresholds of vggn_distance_stats.
 *
 * All arithmetic is float64, without floating-point contraction, and parenthesised as written; a + b + c means (a + b) + c.
 *
 * THE GRID is origin (ox, oy, oz), cell > 0 and dims (d0, d1, d2), each >= 1, with d0 d1 d2 <= 2^25 = VGGN_MAX_CELLS cells.
 *   The cell of a point p:  a point with a non-finite coordinate has cell -1 and takes part in nothing.  Otherwise
 *       t_a = floor((p_a - o_a) / cell),   c_a = clamp(t_a, 0, dims_a - 1),   id = (c_2 dims_1 + c_1) dims_0 + c_0.
 *   A point outside the box lives in the border cell.  That stays correct because the map p_a -> c_a is MONOTONE (a rounded
 *   difference, a rounded quotient by a positive number, floor and clamp each are) and a query's range of cells is clamped the
 *   same way: whatever lies beyond the box on one side is in the border cell of that side, and a range that reaches beyond the
 *   box on that side ends in that border cell.
 *   A POINT GRID is: the cell ids (vggn_point_cells); a STABLE order by cell id; the points gathered into that order
 *   (vggn_gather_points) with their original indices; cell_start (C + 1) int32, cell_start[c] = the number of sorted ids < c
 *   (vggn_cell_start), so the points of cell c are the sorted rows cell_start[c] .. cell_start[c + 1] - 1, in ascending
 *   original index, and the points with cell -1 stand before cell_start[0], where no query looks.
 *
 * NEAREST POINT.  For a query q, r = max_dist > 0 and r2 = r r (computed once by the caller and passed as a double), the
 * candidates are the grid points with a cell >= 0; with exclude_self the candidate whose original index equals the query's
 * index is left out.  For a candidate p:
 *       dx = q_0 - p_0, dy = q_1 - p_1, dz = q_2 - p_2,   d2 = ((dx dx) + (dy dy)) + dz dz;   accepted when d2 <= r2.
 *   index = the original index and dist2 = the d2 of the lexicographic minimum of (d2, original index) over the accepted
 *   candidates (-1 and +inf when there is none, and for a query with a non-finite coordinate); count = the number of accepted
 *   candidates (0 for such a query).  A minimum and an integer count are commutative and associative: the outputs are the same
 *   bits for any traversal order, any order of the points inside a cell and any spread of the work.
 *
 * CANDIDATE CELLS are any superset of the cells that hold an accepted candidate; the result does not depend on the superset.
 * The kernel takes, per axis a,
 *       lo_a = clamp(floor(((q_a - r) - o_a) / cell) - 1, 0, dims_a - 1),
 *       hi_a = clamp(floor(((q_a + r) - o_a) / cell) + 1, 0, dims_a - 1):
 *   the cells of the corners of the box q +- r by the grid's own map, with a MARGIN OF ONE CELL on either side; and the whole
 *   axis, lo_a = 0, hi_a = dims_a - 1, unless |q_a| < 2^40 cell and r < 2^40 cell.
 *   Why one cell is enough.  With u = 2^-53: d2 <= r2 gives (dx dx)(1 - u)^2 <= r r (1 + u), so |dx| <= r (1 + 2 u), and dx
 *   is the rounded q_a - p_a, so |q_a - p_a| <= r (1 + 4 u).  x = the rounded q_a - r is at most (q_a - r) + u |q_a - r|.
 *   Either p_a >= x, and then c(p_a) >= c(x) by monotonicity with no margin at all; or p_a < x with
 *   x - p_a <= delta = u (5 r + |q_a|) < 2^-10 cell under the condition above.  Then the rounded differences x - o_a and
 *   p_a - o_a are at most delta + 2 u |x - o_a| apart and the rounded quotients T at most (delta / cell)(1 + u) + 4 u |T(x)|.
 *   Where |T(x)| < 2^26 that is below 1, so the floors differ by at most one cell: the margin.  Where |T(x)| >= 2^26, T(p_a) is
 *   beyond the box on the same side (dims_a <= 2^25) and both are clamped to the same border cell.  The other side mirrors
 *   this.  For the nearest triangle the same holds of the closest point, which lies in the face's box (below) up to the
 *   rounding of its own few operations, orders of magnitude inside the 2^-10 cell that the condition leaves.
 *   A row of cells (c_0 = lo_0 .. hi_0 at fixed c_1, c_2) is contiguous in the sorted arrays: one loop per row.
 *
 * THE TRIANGLE GRID of vertices (V, 3) doubles and faces (F, 3) int32.  A face is skipped when a row is outside [0, V) (no
 * load is made there), two rows are equal, a vertex coordinate is not finite, or, with ab = b - a, ac = c - a,
 *       n = (ab_1 ac_2 - ab_2 ac_1,  ab_2 ac_0 - ab_0 ac_2,  ab_0 ac_1 - ab_1 ac_0),   ((n_0 n_0) + (n_1 n_1)) + n_2 n_2
 *   is not > 0.  A valid face is registered in every cell of the box c_a(min(a_a, b_a, c_a)) .. c_a(max(a_a, b_a, c_a)), a =
 *   0, 1, 2 (by monotonicity every point of the triangle has its cell there).  The pair list: a per-face count
 *   (vggn_face_cell_counts; 0 for a skipped face), an exclusive sum (the caller's), the (cell, face) pairs written face by
 *   face, the cells of a face in row-major order, c_0 fastest (vggn_face_cell_pairs), a stable sort by cell (the caller's),
 *   cell_start over the sorted cells (vggn_cell_start).  At most 2^31 - 1 pairs.
 *
 * NEAREST TRIANGLE.  The closest point of triangle (a, b, c) to q, after Ericson, Real-Time Collision Detection, 5.1.5, with
 * dot(x, y) = ((x_0 y_0) + (x_1 y_1)) + x_2 y_2 and the regions tested in this order (the first that holds decides):
 *       ab = b - a, ac = c - a, ap = q - a;  d1 = dot(ab, ap), d2 = dot(ac, ap);
 *   A:        d1 <= 0 and d2 <= 0                                   ->  a
 *       bp = q - b;  d3 = dot(ab, bp), d4 = dot(ac, bp);
 *   B:        d3 >= 0 and d4 <= d3                                  ->  b
 *       vc = (d1 d4) - (d3 d2);
 *   AB:       vc <= 0 and d1 >= 0 and d3 <= 0;  v = d1 / (d1 - d3)  ->  a_i + v ab_i
 *       cp = q - c;  d5 = dot(ab, cp), d6 = dot(ac, cp);
 *   C:        d6 >= 0 and d5 <= d6                                  ->  c
 *       vb = (d5 d2) - (d1 d6);
 *   AC:       vb <= 0 and d2 >= 0 and d6 <= 0;  w = d2 / (d2 - d6)  ->  a_i + w ac_i
 *       va = (d3 d6) - (d5 d4);  e = d4 - d3,  f = d5 - d6;
 *   BC:       va <= 0 and e >= 0 and f >= 0;  w = e / (e + f)       ->  b_i + w (c_i - b_i)
 *   interior: den = 1 / ((va + vb) + vc), v = vb den, w = vc den     ->  (a_i + ab_i v) + ac_i w.
 *   With x the closest point, dx = q_0 - x_0 and so on, d2 as for points, accepted when d2 <= r2.  face and dist2 are those of
 *   the lexicographic minimum of (d2, face index) over the accepted faces (-1, +inf without one); closest (optional) is its x,
 *   NaN without one.  A face met in several cells gives the same d2 each time, so meeting it again changes nothing.
 *
 * STATISTICS.  Over dist2 (M): found = #{d2 finite}; below_k = #{sqrt(d2) < tau_k}, k < K <= VGGN_MAX_THRESHOLDS; sum_d = the
 * sum of sqrt(d2) and sum_d2 the sum of d2 over the found entries.  The order of the sums is fixed: VGGN_STATS_GROUPS
 * workgroups of one wavefront of 64 lanes (a constant, not the device's CU count); lane l of group g adds its entries
 * i = 64 g + l, + 64 VGGN_STATS_GROUPS, ... in ascending i, starting from 0; the 64 lane sums are added by the xor butterfly
 * of common.hpp (offsets 32, 16, 8, 4, 2, 1); a last launch adds the VGGN_STATS_GROUPS partials in ascending g, starting from
 * 0.  Two runs on any gfx950 give the same bits.  The counts are integers.
 *
 * What is a kernel and what is the caller's (torch, in vggsfm_amd/nearest.py): the caller allocates, sorts the cell ids
 * (one stable sort of int32 keys per grid and one per set of queries), takes the exclusive sum of the per-face counts and
 * gathers the face column of the sorted pairs.  Everything else is an entry of this header.
 */
#ifndef VGGSFM_AMD_NN_H
#define VGGSFM_AMD_NN_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VGGN_MAX_CELLS 33554432    /* 2^25 cells to a grid */
#define VGGN_MAX_THRESHOLDS 8      /* thresholds to a call of vggn_distance_stats */
#define VGGN_STATS_GROUPS 256      /* wavefronts (workgroups of 64 lanes) of the statistics, whatever the device */
#define VGGN_STATS_WORDS 12        /* 8-byte words per group in the statistics' workspace */

const char* vggn_build_arch(void);

/* Every entry that takes a grid refuses: cell not > 0 (a NaN is refused), a dim < 1, more than VGGN_MAX_CELLS cells. */

/* out_cell (n) int32 = the cell id of each point (n, 3), -1 for a non-finite one.  One lane per point.  Refused: n < 0.
 * n = 0 is a no-op. */
int vggn_point_cells(const double* points, int n, double ox, double oy, double oz, double cell, int d0, int d1, int d2,
                     int32_t* out_cell, void* stream);

/* out_points[i] = points[order[i]], i < n; order (n) int32, a permutation of 0 .. n - 1 (a row outside [0, n) is not
 * loaded; its output is NaN).  Refused: n < 0.  n = 0 is a no-op. */
int vggn_gather_points(const double* points, const int32_t* order, int n, double* out_points, void* stream);

/* cell_start (num_cells + 1) int32: cell_start[c] = the number of entries of sorted_cell (n, ascending) that are < c, by a
 * binary search per cell.  Refused: n < 0, num_cells < 1 or > VGGN_MAX_CELLS.  With n = 0 every entry is 0. */
int vggn_cell_start(const int32_t* sorted_cell, int n, int num_cells, int32_t* cell_start, void* stream);

/* NEAREST POINT.  grid_points (n, 3) and grid_index (n) are the sorted points and their original indices, cell_start that of
 * their cells.  visit (m) int32: lane j serves query visit[j] and writes at visit[j]; the caller passes the order of the
 * queries' own cells, so that the lanes of a wavefront walk the same few cells (an entry outside [0, m) is ignored).
 * out_index (m) int32, out_dist2 (m) doubles, out_count (m) int32 or NULL.  One lane per query, no LDS, no atomic.
 * Refused: max_dist not > 0 (a NaN is refused), r2 not >= 0, n < 0, m < 0.  m = 0 is a no-op; with n = 0 every query gets
 * "none" (-1, +inf, 0). */
int vggn_nearest_point(const double* grid_points, const int32_t* grid_index, const int32_t* cell_start, int n, double ox,
                       double oy, double oz, double cell, int d0, int d1, int d2, const double* queries,
                       const int32_t* visit, int m, double max_dist, double r2, int exclude_self, int32_t* out_index,
                       double* out_dist2, int32_t* out_count, void* stream);

/* out_count (num_faces) int32 = the number of cells each face is registered in, 0 for a skipped face.  One lane per face.
 * Refused: num_vertices < 0, num_faces < 0.  num_faces = 0 is a no-op. */
int vggn_face_cell_counts(const double* vertices, int num_vertices, const int32_t* faces, int num_faces, double ox, double oy,
                          double oz, double cell, int d0, int d1, int d2, int32_t* out_count, void* stream);

/* offset (num_faces) int64 = the exclusive sum of the counts.  Face g writes its pairs at offset[g] ..: pair_cell and
 * pair_face (num_pairs) int32.  A face whose pairs would not fit below num_pairs writes none.  One lane per face.
 * Refused: num_vertices < 0, num_faces < 0, num_pairs < 0 or > 2^31 - 1.  num_faces = 0 or num_pairs = 0 is a no-op. */
int vggn_face_cell_pairs(const double* vertices, int num_vertices, const int32_t* faces, int num_faces, double ox, double oy,
                         double oz, double cell, int d0, int d1, int d2, const int64_t* offset, long num_pairs,
                         int32_t* pair_cell, int32_t* pair_face, void* stream);

/* NEAREST TRIANGLE.  cell_faces (num_pairs) int32: the face column of the pairs sorted by cell; cell_start that of the cell
 * column.  visit as for points.  out_face (m) int32, out_dist2 (m) doubles, out_closest (m, 3) doubles or NULL.  A listed
 * face with a row outside [0, V) or outside [0, F) is passed over (no load).  One lane per query, no LDS, no atomic.
 * Refused: max_dist not > 0 (a NaN is refused), r2 not >= 0, a negative num_vertices, num_faces, num_pairs or m.  m = 0 is a
 * no-op; with num_faces = 0 or num_pairs = 0 every query gets "none" (-1, +inf, NaN). */
int vggn_nearest_face(const double* vertices, int num_vertices, const int32_t* faces, int num_faces, const int32_t* cell_faces,
                      const int32_t* cell_start, int num_pairs, double ox, double oy, double oz, double cell, int d0, int d1,
                      int d2, const double* queries, const int32_t* visit, int m, double max_dist, double r2,
                      int32_t* out_face, double* out_dist2, double* out_closest, void* stream);

/* STATISTICS.  thresholds: a HOST array of K doubles (NULL with K = 0).  out_counts (1 + K) int64: found, below_0 ..;
 * out_sums (2) doubles: sum_d, sum_d2.  workspace: VGGN_STATS_GROUPS x VGGN_STATS_WORDS 8-byte words, written and read by the
 * two launches.  Refused: m < 0, K < 0 or > VGGN_MAX_THRESHOLDS, K > 0 without thresholds.  m = 0 writes zeros. */
int vggn_distance_stats(const double* dist2, int m, const double* thresholds, int num_thresholds, int64_t* out_counts,
                        double* out_sums, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif
