/*
 * vggsfm_amd -- registration of a dense model to a reference: ICP on the uniform grid of vggsfm_amd_nn.h, and the normals of
 * a reference scan that has none (libvggsfm_amd_icp.so, a library of its own: the entries of the other libraries and the
 * headers under include/ are closed, counted sets).
 *
 * Conventions of include/vggsfm_amd.h hold: device pointers, `stream` a hipStream_t as void*, asynchronous (no entry
 * synchronises with the host), no allocation, VGG_OK (0) or a negative VGG_ERR_* code; every refusal is decided on the host
 * before a launch.  The names carry the prefix vggi_; their rows stand in vggsfm_amd/_lib_icp.py.  One argument is a HOST
 * array: `toward` of vggi_radius_normals.
 *
 * All arithmetic is float64, without floating-point contraction, and parenthesised as written; a + b + c means (a + b) + c,
 * dot(x, y) = ((x_0 y_0) + (x_1 y_1)) + x_2 y_2, cross(x, y) = (x_1 y_2 - x_2 y_1, x_2 y_0 - x_0 y_2, x_0 y_1 - x_1 y_0).
 *
 * THE GRID, the point grid, the triangle grid, the candidate cells of a query and the closest point of a triangle are those
 * of vggsfm_amd_nn.h, by the same device code (csrc/nn/nn_grid.hpp); the arrays are what nearest.PointGrid / TriangleGrid
 * hold.  A grid is refused as there: cell not > 0, a dim < 1, more than VGGN_MAX_CELLS = 2^25 cells.
 *
 * THE STATE (VGGI_STATE_WORDS doubles on the device): the transform T = (s, R, t) with x = s R p + t, the centre c the
 * increments turn about, a status and the number of updates made.
 *       [0] status   VGGI_RUNNING 0, VGGI_CONVERGED 1, VGGI_TOO_FEW 2, VGGI_DEGENERATE 3   (as a double)
 *       [1] iterations = the number of updates applied                                       (as a double)
 *       [2] s     [3 .. 11] R, row-major     [12 .. 14] t     [15 .. 17] c
 * A step or update kernel whose state's status is not VGGI_RUNNING returns at once and writes nothing.
 *
 * THE STEP, per source point p (queries in the order of `visit`, as vggn_nearest_point):
 *   1. x_i = (s (((R_i0 p_0) + (R_i1 p_1)) + R_i2 p_2)) + t_i.  A non-finite x takes part in nothing.
 *   2. The winner within max_dist by the exact rule of vggsfm_amd_nn.h: with d2 = ((dx dx) + (dy dy)) + dz dz accepted
 *      when d2 <= r2, the lexicographic minimum of (d2, original index) over the accepted grid points (point target), or of
 *      (d2, face index) over the valid faces, d2 taken to the closest point of the face (mesh target).  y = the winning
 *      point, or the closest point of the winning face.
 *   3. The normal n: normals[winner] (point target; not read when `normals` is NULL, which metric 1 refuses unless n = 0), or for a
 *      mesh u = cross(b - a, c - a), n = u / sqrt(dot(u, u)).  A pair whose n has a non-finite component is dropped.
 *      out_index (optional) = the winner of a pair that is kept, -1 otherwise.
 *   4. e = x - y.  metric 0 (point to point): three residual rows k = 0, 1, 2 with r_k = e_k; metric 1 (point to plane): one
 *      row with r = dot(n, e).
 *   5. With z = x - c the Jacobian of x about c in (omega, tau, lambda) is [-[z]x, I, z]; the rows are
 *         metric 0, row k:  J = (row k of -[z]x, row k of I, z_k):
 *                           k = 0: (0, z_2, -z_1, 1, 0, 0, z_0)   k = 1: (-z_2, 0, z_0, 0, 1, 0, z_1)   k = 2: (z_1, -z_0, 0, 0, 0, 1, z_2)
 *         metric 1:         J = (cross(z, n), n, dot(n, z)).
 *      Without estimate_scale J_6 = 0.
 *   6. rho = |r| (metric 1) or sqrt(dot(e, e)) (metric 0); k = loss_scale.  The weight w:
 *         loss 0: 1;   loss 1 (Huber): 1 when rho <= k, else k / rho;
 *         loss 2 (Tukey): q = rho / k, v = 1 - (q q), w = v v when rho < k, else 0.
 *   Accumulated over the kept pairs, each word starting from 0 and row by row in the order k = 0, 1, 2:
 *         H_ij += (w J_i) J_j  (i <= j: 28 words, row-major upper triangle),   g_i += (w J_i) r  (7 words),
 *         sum_w += w,   sum_wr2 += w R2,   sum_r2 += R2   with R2 = r r (metric 1) or dot(e, e) (metric 0),   count += 1.
 *   THE ORDER OF THE SUMS is fixed: VGGI_GROUPS workgroups of VGGI_BLOCK lanes (constants, not the device's CU count);
 *   lane l of group b takes the visit positions j = VGGI_BLOCK b + l, + VGGI_BLOCK VGGI_GROUPS, ... in ascending j; the 64
 *   lane sums of a wavefront are added by the xor butterfly of crosslane.hpp (offsets 32, 16, 8, 4, 2, 1); the wavefronts of
 *   a group are added in ascending order, starting from wavefront 0's sum, through LDS; each group writes one row of
 *   VGGI_WORDS 8-byte words into the workspace:  [0 .. 27] H, [28 .. 34] g, [35] sum_w, [36] sum_wr2, [37] sum_r2,
 *   [38] count as int64, [39] 0.  No atomic.  vggi_icp_sums and vggi_icp_update add the rows in ascending group order,
 *   starting from 0.  Two runs on any gfx950 give the same bits; the visit order moves the last bits of the sums and
 *   nothing else.
 *
 * THE UPDATE (one wavefront).  n = 7 with estimate_scale, else 6.
 *   count < min_correspondences                           -> status VGGI_TOO_FEW, nothing else changes.
 *   some H_ii (i < n) not > 0                              -> status VGGI_DEGENERATE.
 *   d_i = 1 / sqrt(H_ii);  A_ij = (H_ij d_i) d_j (i < j),  A_ii = 1 + damping;  b_i = -(g_i d_i).
 *   Cholesky A = L L^T, column by column: p_j = A_jj - sum_{k<j} L_jk L_jk (k ascending);  p_j not > VGGI_PIVOT_MIN ->
 *   VGGI_DEGENERATE;  L_jj = sqrt(p_j),  L_ij = (A_ij - sum_{k<j} L_ik L_jk) / L_jj.  Forward and back substitution in
 *   ascending / descending order give y;  delta_i = y_i d_i = (omega, tau, lambda), lambda = 0 without estimate_scale.
 *   Exp(omega) by Rodrigues: th2 = dot(omega, omega), th = sqrt(th2);
 *         th2 < 1e-8:  A = 1 - th2 / 6,  B = 0.5 - th2 / 24;   else  A = sin(th) / th,  h = sin(0.5 th),  B = (2 (h h)) / th2;
 *         E = I + A [omega]x + B (omega omega^T - th2 I).
 *   R <- E R;   t <- (c + (1 + lambda) (E (t - c))) + tau;   s <- s (1 + lambda);   iterations += 1.
 *   history (optional, (history_rows, VGGI_HISTORY_WORDS) doubles): row `iterations` (before the increment, when below
 *   history_rows) = count, sum_w, sum_wr2, sum_r2, |omega|, |tau|, lambda: the sums are those AT the transform the update
 *   started from.
 *   status VGGI_CONVERGED when |omega| <= rotation_tol and |tau| <= translation_tol and |lambda| <= scale_tol.
 *   A run of K iterations is K x (step, update) enqueued back to back; once the status leaves VGGI_RUNNING the rest do nothing.
 *
 * RADIUS NORMALS of a point grid, one lane per grid point q (finite): the neighbours are the grid points with
 * d2 <= r2 (q itself among them), met in the kernel's traversal order (rows of cells c_2, c_1 ascending, sorted rows
 * ascending inside).  count = their number.  Pass 1: mean m = (sum of p) / count.  Pass 2: C = (sum of (p - m)(p - m)^T) /
 * count.  The cyclic Jacobi solver of csrc/jacobi.hpp (jacobi_sym3, VGGI_NORMAL_SWEEPS sweeps) leaves eigenvalues a_0, a_1, a_2
 * on the diagonal and their vectors; the normal is the vector of the smallest a_b (the first minimum) divided by its length,
 * negated when dot(n, toward - q) < 0 with a viewpoint, else when its first non-zero component is negative; curvature =
 * a_b / ((a_0 + a_1) + a_2).  With
 * count < min_neighbors, or a non-finite point: normal NaN, curvature NaN (count still written, 0 for a non-finite point).
 * The outputs stand at the point's ORIGINAL index.
 */
#ifndef VGGSFM_AMD_ICP_H
#define VGGSFM_AMD_ICP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef VGGI_GROUPS                /* (a measurement build of scripts/time_icp.py may set the two; the library's are these) */
#define VGGI_GROUPS 512            /* workgroups of the step, whatever the device */
#define VGGI_BLOCK 256             /* lanes to a workgroup of the step: 64, 128, 256 or 512 */
#endif
#define VGGI_WORDS 40              /* 8-byte words per group in the workspace, and of vggi_icp_sums' output */
#define VGGI_STATE_WORDS 18
#define VGGI_HISTORY_WORDS 7
#define VGGI_NORMAL_SWEEPS 8
#define VGGI_PIVOT_MIN 1e-12       /* the smallest pivot of the Jacobi-scaled normal equations */
#define VGGI_RUNNING 0
#define VGGI_CONVERGED 1
#define VGGI_TOO_FEW 2
#define VGGI_DEGENERATE 3

const char* vggi_build_arch(void);

/* THE STEP against a point grid.  source (m, 3); visit (m) int32 (an entry outside [0, m) is ignored); grid_points (n, 3),
 * grid_index (n), cell_start: the sorted points, their original indices and the cells' starts; normals (n, 3) in ORIGINAL
 * index order, or NULL; state (VGGI_STATE_WORDS); workspace VGGI_GROUPS x VGGI_WORDS 8-byte words; out_index (m) int32 or
 * NULL.  Refused: a bad grid, max_dist not > 0 (a NaN is refused), r2 not >= 0, n < 0, m < 0, metric not 0 or 1, metric 1
 * without normals (unless n = 0), loss not 0, 1 or 2, loss 1 or 2 with loss_scale not > 0, a missing state or workspace.  m = 0 and n = 0 are
 * launched: the sums are zeros. */
int vggi_icp_step(const double* source, const int32_t* visit, int m, const double* grid_points, const int32_t* grid_index,
                  const int32_t* cell_start, int n, double ox, double oy, double oz, double cell, int d0, int d1, int d2,
                  const double* normals, const double* state, double max_dist, double r2, int metric, int estimate_scale,
                  int loss, double loss_scale, void* workspace, int32_t* out_index, void* stream);

/* THE STEP against a triangle grid: the arrays of vggn_nearest_face.  Refused as above (no normals argument), and a negative
 * num_vertices, num_faces or num_pairs. */
int vggi_icp_step_mesh(const double* source, const int32_t* visit, int m, const double* vertices, int num_vertices,
                       const int32_t* faces, int num_faces, const int32_t* cell_faces, const int32_t* cell_start,
                       int num_pairs, double ox, double oy, double oz, double cell, int d0, int d1, int d2,
                       const double* state, double max_dist, double r2, int metric, int estimate_scale, int loss,
                       double loss_scale, void* workspace, int32_t* out_index, void* stream);

/* out (VGGI_WORDS 8-byte words, the layout of a workspace row) = the rows of the workspace added in ascending group order.
 * One wavefront.  Reads no state: it runs whatever the status.  Refused: a missing pointer. */
int vggi_icp_sums(const void* workspace, void* out, void* stream);

/* THE UPDATE.  history (history_rows, VGGI_HISTORY_WORDS) or NULL with history_rows = 0.  Refused: a missing workspace or
 * state, min_correspondences < 1, damping not >= 0, a tolerance that is NaN, history_rows < 0, history_rows > 0 without
 * history. */
int vggi_icp_update(const void* workspace, double* state, int estimate_scale, int min_correspondences, double damping,
                    double rotation_tol, double translation_tol, double scale_tol, double* history, int history_rows,
                    void* stream);

/* RADIUS NORMALS.  toward: a HOST array of 3 doubles, or NULL.  out_normal (n, 3), out_curvature (n) doubles, out_count (n)
 * int32.  Refused: a bad grid, n < 0, radius not > 0, r2 not >= 0, min_neighbors < 1, a non-finite toward.  n = 0 is a
 * no-op. */
int vggi_radius_normals(const double* grid_points, const int32_t* grid_index, const int32_t* cell_start, int n, double ox,
                        double oy, double oz, double cell, int d0, int d1, int d2, double radius, double r2,
                        int min_neighbors, const double* toward, double* out_normal, double* out_curvature,
                        int32_t* out_count, void* stream);

#ifdef __cplusplus
}
#endif
#endif
