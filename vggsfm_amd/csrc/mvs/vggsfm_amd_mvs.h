/*
 * vggsfm_amd -- plane-sweep multi-view stereo: dense depth of one view from its neighbours and the forward-backward
 * consistency check of the depth maps (libvggsfm_amd_mvs.so, a library of its own: the entries of libvggsfm_amd.so and
 * the headers under include/ are a closed, counted set, and so are the tracker's).
 *
 * Conventions of include/vggsfm_amd.h hold: device pointers, `stream` a hipStream_t as void*, asynchronous (no entry
 * synchronises with the host), no allocation, VGG_OK (0) or a negative VGG_ERR_* code.  The names carry the prefix vggm_;
 * their rows stand in vggsfm_amd/_lib_mvs.py.  Two arguments are HOST arrays, read before the entry returns, so that the
 * entry can refuse them: `sources` and `ray_index` (a handful of int32 each).
 *
 * Images are float32, row-major; a point (x, y) with integer coordinates is the centre of pixel [y][x].  poses (S, 3, 4)
 * doubles [R|t], camera from world; cams (S, 4) doubles f, cx, cy, k (k = 0: SIMPLE_PINHOLE, else SIMPLE_RADIAL).  A ray
 * map (H, W, 2) doubles holds per pixel centre its undistorted normalised coordinates (u, v): the point (u, v, 1) z of the
 * camera frame projects to the pixel for every z > 0.
 *
 * All arithmetic is float64 from the float32 pixels and depths, without floating-point contraction; a + b + c means
 * (a + b) + c.  Every sum is taken in a fixed order and there are no atomics: two runs give the same bits.
 * A frame of 0 pixels is a no-op that returns VGG_OK.
 *
 * Shared by both entries:
 *   relative pose of b from a:  R[i][j] = Rb[i][0] Ra[j][0] + Rb[i][1] Ra[j][1] + Rb[i][2] Ra[j][2],
 *                               t[i] = tb[i] - (R[i][0] ta[0] + R[i][1] ta[1] + R[i][2] ta[2]);
 *   transfer of P:              X[i] = R[i][0] P[0] + R[i][1] P[1] + R[i][2] P[2] + t[i];
 *   projection of X (X[2] > 0): iz = 1 / X[2], a = X[0] iz, b = X[1] iz, d = 1 + k (a a + b b),
 *                               x = f (a d) + cx, y = f (b d) + cy.
 */
#ifndef VGGSFM_AMD_MVS_H
#define VGGSFM_AMD_MVS_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VGGM_MAX_SOURCES 8
#define VGGM_MAX_PLANES 1024
#define VGGM_MAX_RADIUS 3

const char* vggm_build_arch(void);

/* Plane sweep of view `ref` of frames (num_frames, height, width) against sources[0 .. num_sources) (HOST int32, each in
 * [0, num_frames) and not ref; 1 <= num_sources <= 8).  rays: the ray map of view ref.  Refused: num_planes outside
 * 1 .. 1024, radius outside 1 .. 3, min_views outside 1 .. num_sources, not 0 < inv_depth_far < inv_depth_near (both finite).
 *
 * Planes: dw = (inv_depth_near - inv_depth_far) / (num_planes - 1) (0 for one plane), w_j = inv_depth_far + j dw.
 * Window of pixel (x, y): k = 0 .. n - 1, n = (2 radius + 1)^2, row-major, dy outside and dx inside, window pixel
 * (clamp(x + dx, 0, W - 1), clamp(y + dy, 0, H - 1)); A_k its intensity in view ref, (u_k, v_k) its ray.
 * Reference window: mA = (sum_k A_k) / n; a_k = A_k - mA; sa = sum_k a_k; taa = sum_k a_k a_k - sa sa / n.  A pixel with
 * not (taa / n >= min_variance) has cost +inf on every plane.
 * Source m (relative pose of sources[m] from ref, its f, cx, cy, k) on plane j, with q = 1 / w_j: window pixel k is
 * transferred as P = (u_k q, v_k q, q) and projected.  It is outside when X[2] <= 0 or not (0 <= x <= W - 1 and
 * 0 <= y <= H - 1); a source with a window pixel outside is invalid for this pixel and plane.  Otherwise B_k is the
 * bilinear sample of the source frame at (x, y): x0 = floor(x), x1 = min(x0 + 1, W - 1), fx = x - x0, likewise y,
 *   B_k = ((1 - fx) (1 - fy)) I[y0][x0] + (fx (1 - fy)) I[y0][x1] + ((1 - fx) fy) I[y1][x0] + (fx fy) I[y1][x1],
 * b_k = B_k - mA, sb = sum_k b_k, sbb = sum_k b_k b_k, sab = sum_k a_k b_k (all over k ascending),
 *   tbb = sbb - sb sb / n, tab = sab - sa sb / n, den = sqrt(taa tbb), zncc = tab / den if den > 0, else 0
 * (a source window without variance scores 0 and counts).
 * cost_j = (sum over the valid sources in list order of (1 - zncc)) / (their number), +inf with fewer than min_views.
 *
 * Selection: the best plane j has the lowest finite cost c, ties to the lowest j; none: depth 0, conf 0, index -1.
 * With 0 < j < num_planes - 1, both neighbours' costs cm, cp finite and e = cm - 2 c + cp > 0:
 * w = w_j + ((0.5 (cm - cp)) / e) dw, else w = w_j.  conf = 1 - c; conf < min_conf: depth 0 and index -1 (conf is
 * written); else depth = 1 / w, index = j.
 *
 * out_depth, out_conf (height, width) float32 (rounded from the doubles), out_index (height, width) int32,
 * out_cost (num_planes, height, width) doubles or NULL. */
int vggm_plane_sweep(const float* frames, const double* poses, const double* cams, const double* rays, int num_frames,
                     int height, int width, int ref, const int32_t* sources, int num_sources, double inv_depth_far,
                     double inv_depth_near, int num_planes, int radius, int min_views, double min_variance, double min_conf,
                     float* out_depth, float* out_conf, int32_t* out_index, double* out_cost, void* stream);

/* Forward-backward check of the depth map of view `ref` of depth (num_frames, height, width), 0 = no depth, against the
 * maps of sources[0 .. num_sources) (HOST int32, as above).  rays (num_rays, height, width, 2): ray maps; view s uses
 * map ray_index[s] (HOST int32 (num_frames), each in [0, num_rays)).  Refused: min_consistent < 1, a negative or NaN tolerance.
 *
 * Pixel (x, y) of view ref with z = depth > 0 and ray (u, v): P = (u z, v z, z) is transferred to source m (relative pose
 * of sources[m] from ref) and projected with the source's camera to (xs, ys).  Not consistent when X[2] <= 0 or, with
 * xi = floor(xs + 0.5), yi = floor(ys + 0.5) (the nearest pixel, halves up), not (0 <= xi <= W - 1 and 0 <= yi <= H - 1),
 * or the source's depth zs at [yi][xi] is not > 0.  Else Q = (us zs, vs zs, zs) with the source's ray at [yi][xi] is
 * transferred back (relative pose of ref from sources[m]) to Y and, with Y[2] > 0, projected with the camera of ref to
 * (xb, yb); the source is consistent when sqrt((xb - x)^2 + (yb - y)^2) <= reproj_tol and
 * |Y[2] - z| / z <= rel_depth_tol.
 * out_count (height, width) int32: the number of consistent sources (0 where z is not > 0); out_depth (height, width)
 * float32: z where out_count >= min_consistent, else 0. */
int vggm_consistency_filter(const float* depth, const double* poses, const double* cams, const double* rays,
                            const int32_t* ray_index, int num_rays, int num_frames, int height, int width, int ref,
                            const int32_t* sources, int num_sources, double rel_depth_tol, double reproj_tol,
                            int min_consistent, float* out_depth, int32_t* out_count, void* stream);

#ifdef __cplusplus
}
#endif
#endif
