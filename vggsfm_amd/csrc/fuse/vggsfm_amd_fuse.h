/*
 * vggsfm_amd -- fusion of the depth maps of a reconstruction into one point cloud: per-pixel normals of the maps and the
 * view-by-view fusion with de-duplication and an ordered output (libvggsfm_amd_fuse.so, a library of its own: the entries
 * of the other libraries and the headers under include/ are closed, counted sets).
 *
 * Conventions of include/vggsfm_amd.h hold: device pointers, `stream` a hipStream_t as void*, asynchronous (no entry
 * synchronises with the host), no allocation, VGG_OK (0) or a negative VGG_ERR_* code.  The names carry the prefix vggf_;
 * their rows stand in vggsfm_amd/_lib_fuse.py.  Two arguments are HOST arrays, read before the entry returns, so that the
 * entry can refuse them before a kernel indexes with them: `sources` and `ray_index` (a handful of int32 each).
 *
 * Maps are row-major; a point (x, y) with integer coordinates is the centre of pixel [y][x].  depth (S, H, W) float32,
 * 0 = no depth.  poses (S, 3, 4) doubles [R|t], camera from world; cams (S, 4) doubles f, cx, cy, k (k = 0:
 * SIMPLE_PINHOLE, else SIMPLE_RADIAL).  rays (num_rays, H, W, 2) doubles: ray maps, per pixel centre its undistorted
 * normalised coordinates (u, v); view s uses map ray_index[s] (HOST int32 (S), each in [0, num_rays)).
 *
 * All arithmetic is float64 from the float32 inputs, without floating-point contraction; a + b + c means (a + b) + c.
 * Every sum is taken in a fixed order; no atomic decides a value or an order: two runs give the same bits.
 * A frame of 0 pixels is a no-op that returns VGG_OK.
 *
 * Shared with the stereo (one copy, csrc/mvs/mvs_geometry.hpp):
 *   relative pose of b from a:  R[i][j] = Rb[i][0] Ra[j][0] + Rb[i][1] Ra[j][1] + Rb[i][2] Ra[j][2],
 *                               t[i] = tb[i] - (R[i][0] ta[0] + R[i][1] ta[1] + R[i][2] ta[2]);
 *   transfer of P:              X[i] = R[i][0] P[0] + R[i][1] P[1] + R[i][2] P[2] + t[i];
 *   projection of X (X[2] > 0): iz = 1 / X[2], a = X[0] iz, b = X[1] iz, d = 1 + k (a a + b b),
 *                               x = f (a d) + cx, y = f (b d) + cy.
 * Here alone, with [R|t] the pose of a view:
 *   world point of P:           Q[i] = P[i] - t[i],  X[i] = R[0][i] Q[0] + R[1][i] Q[1] + R[2][i] Q[2];
 *   world direction of n:       w[i] = R[0][i] n[0] + R[1][i] n[1] + R[2][i] n[2].
 */
#ifndef VGGSFM_AMD_FUSE_H
#define VGGSFM_AMD_FUSE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VGGF_MAX_SOURCES 8

const char* vggf_build_arch(void);

/* Normals of every depth map: out_normals (S, H, W, 3) float32 in the world frame, (0, 0, 0) = no normal.  Views go 256 to
 * a launch.  Refused: max_rel_jump negative or NaN, a ray index outside [0, num_rays), num_rays < 1, num_frames < 1.
 *
 * Pixel (x, y) of view s with z = depth > 0 and ray (u, v) has the camera-frame point P = (u z, v z, z); z not > 0: no
 * normal.  A neighbour pixel counts when it lies in the frame, its depth zn is > 0 and |zn - z| <= max_rel_jump z.
 * gx = P(x + 1, y) - P(x - 1, y) when both neighbours count, else P(x + 1, y) - P when the right one counts, else
 * P - P(x - 1, y) when the left one counts, else there is no normal; gy likewise with (x, y + 1) and (x, y - 1).
 * n = gx x gy:  n[0] = gx[1] gy[2] - gx[2] gy[1],  n[1] = gx[2] gy[0] - gx[0] gy[2],  n[2] = gx[0] gy[1] - gx[1] gy[0];
 * len = sqrt(n[0] n[0] + n[1] n[1] + n[2] n[2]),  d = n[0] P[0] + n[1] P[1] + n[2] P[2].  No normal unless len > 0 and
 * d != 0 (a NaN is no normal).  m[i] = n[i] / len, negated when d > 0 (the normal faces the camera: m . P < 0); the
 * output is the world direction of m, rounded once to float32. */
int vggf_depth_normals(const float* depth, const double* poses, const double* rays, const int32_t* ray_index, int num_rays,
                       int num_frames, int height, int width, double max_rel_jump, float* out_normals, void* stream);

/* Fuses view `view` into the cloud: the pixels of the view that no earlier view has claimed become points, each the mean
 * of the pixel and of the pixels of sources[0 .. num_sources) (HOST int32, each in [0, num_frames) and not `view`;
 * 0 <= num_sources <= 8) that confirm it.  The caller runs the views in an order of its choice, one call each, with
 * `claimed` (S, H, W) uint8 zeroed before the first call and count_in of a call the count_out of the call before (0
 * before the first).  normals (S, H, W, 3) float32 as vggf_depth_normals writes them, or NULL: no normal test, out_normal
 * not written.  frames (S, 3, H, W) float32 planar colours, or NULL: out_rgb not written.  Refused: view or a source
 * outside [0, num_frames), a source equal to view, num_sources outside 0 .. 8, min_views outside 1 .. num_sources + 1, a
 * negative or NaN rel_depth_tol or reproj_tol, a NaN min_normal_cos, a ray index outside [0, num_rays), capacity < 0.
 *
 * Seed: pixel (x, y) of `view` with z = depth > 0 and claimed[view][y][x] == 0; nv its normal, P = (u z, v z, z).
 * Source m, in list order, exactly as vggm_consistency_filter tests it: P is transferred to the source (relative pose of
 * sources[m] from view) and projected with the source's camera to (xs, ys).  Not consistent when X[2] <= 0 or, with
 * xi = floor(xs + 0.5), yi = floor(ys + 0.5) (the nearest pixel, halves up), not (0 <= xi <= W - 1 and 0 <= yi <= H - 1),
 * or the source's depth zs at [yi][xi] is not > 0.  Else Q = (us zs, vs zs, zs) with the source's ray at [yi][xi] is
 * transferred back (relative pose of view from sources[m]) to Y and, with Y[2] > 0, projected with the camera of view to
 * (xb, yb); required: sqrt((xb - x)^2 + (yb - y)^2) <= reproj_tol and |Y[2] - z| / z <= rel_depth_tol.  With normals,
 * and when both nv and the source pixel's normal ns are not (0, 0, 0), also ns[0] nv[0] + ns[1] nv[1] + ns[2] nv[2] >=
 * min_normal_cos; a pixel without a normal passes.  No load is made at a coordinate that is not used.
 *
 * Contributors: the seed, then the consistent sources in list order; a source contributes the world point of Q under its
 * own pose, ns, and its colour at [yi][xi].  num_views = their number; the pixel emits a point when num_views >=
 * min_views.  xyz = (sum of the world points, in that order) / num_views.  normal: sum of the contributors' normals that
 * are not (0, 0, 0), in that order, t; l = sqrt(t[0] t[0] + t[1] t[1] + t[2] t[2]); t[i] / l rounded to float32 when
 * l > 0, else (0, 0, 0).  rgb[c] = (sum of the contributors' colours of channel c, in that order) / num_views, rounded to
 * float32.
 *
 * Claims: a pixel that emits stores 1 to claimed[s][yi][xi] of each of its consistent sources.  A claimed pixel still
 * supports other seeds; it only cannot be a seed.  The lanes of a call read claimed[view] only and write claimed[s] with
 * s != view only (a source equal to view is refused), and every store writes the same value 1: no race can change a
 * result.
 *
 * Order: the points of a call follow those of the calls before, row-major inside the view; point i of this call goes to
 * row count_in[0] + i of the outputs, and count_out[0] = count_in[0] + (the number of points of this call).  The order
 * comes from counting: a ballot and the bits below the lane per wavefront, the wavefronts' counts per workgroup, the
 * workgroups' counts before a workgroup across the launch -- integer sums, no cursor.  count_in and count_out are device
 * int64 and must not be the same address.  A row >= capacity is not written (count_out still counts it).
 * Outputs per point: out_xyz (capacity, 3) doubles, out_normal, out_rgb (capacity, 3) float32, out_num_views, out_view
 * (= view), out_pixel (= y W + x) (capacity) int32.
 *
 * Workspace, written and read inside the call: stage_views (H W) int32, stage_xyz (H W, 3) doubles, stage_normal,
 * stage_rgb (H W, 3) float32 (either may be NULL when its output is off), block_counts (ceil(H W / 256)) int32. */
int vggf_fuse_view(const float* depth, const float* normals, const float* frames, const double* poses, const double* cams,
                   const double* rays, const int32_t* ray_index, int num_rays, int num_frames, int height, int width,
                   int view, const int32_t* sources, int num_sources, double rel_depth_tol, double reproj_tol,
                   double min_normal_cos, int min_views, uint8_t* claimed, int32_t* stage_views, double* stage_xyz,
                   float* stage_normal, float* stage_rgb, int32_t* block_counts, const int64_t* count_in, int64_t* count_out,
                   long capacity, double* out_xyz, float* out_normal, float* out_rgb, int32_t* out_num_views,
                   int32_t* out_view, int32_t* out_pixel, void* stream);

#ifdef __cplusplus
}
#endif
#endif
