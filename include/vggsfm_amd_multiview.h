/*
 * vggsfm_amd -- masked multi-view triangulation and its helpers (second header of libvggsfm_amd.so).
 *
 * The building blocks of the reference's triangulation as entries of their own:
 *   triangulate_multi_view_point_batched        vggsfm/utils/triangulation_helpers.py:27-131
 *   calculate_normalized_angular_error_batched  vggsfm/utils/triangulation_helpers.py:431-472
 *   calculate_triangulation_angle_batched       vggsfm/utils/triangulation_helpers.py:475-521
 *   calculate_triangulation_angle(_exhaustive)  vggsfm/utils/triangulation_helpers.py:524-587
 *   local_refinement_tri                        vggsfm/utils/triangulation_helpers.py:648-725
 *   triangulate_multi_view_point_from_tracks    vggsfm/utils/triangulation.py:650-674
 * Conventions of include/vggsfm_amd.h hold: device pointers, `stream` a hipStream_t as void*, asynchronous, no
 * allocation, VGG_OK (0) or a negative VGG_ERR_* code.  The names carry the prefix vggx_; their rows in
 * vggsfm_amd/_lib.py stand under this header's key of HEADERS.  All arithmetic is float64, compiled without
 * floating-point contraction; no floating-point atomics: every result is a function of its own point alone, whatever else is in the launch.
 *
 * "Problem" q of n: one DLT solve.  Its cameras and observations belong to group q / group_div; with cam_groups == 1 all
 * problems share ONE camera set (S,3,4) (wave-uniform loads), otherwise cams is (cam_groups,S,3,4) and
 * cam_groups * group_div >= n.
 */
#ifndef VGGSFM_AMD_MULTIVIEW_H
#define VGGSFM_AMD_MULTIVIEW_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* device bytes of `workspace` below: the projection centres -R^T t of every camera, (cam_groups,S,3) f64 */
size_t vggx_multiview_workspace_bytes(long cam_groups, int S);

/* projection centres of `count` cameras (count,3,4) -> out_centers (count,3) */
int vggx_view_centers(const double* cams, long count, double* out_centers, void* stream);

/* n masked DLT solves.  Observation (u,v) of view s of problem q: tracks[(q / group_div) * track_stride_q + s *
 * track_stride_s + {0,1}] (strides in scalars, both even; float32 or float64).  Weight of it: 1 (weight_kind 0), or
 * weights[row * weight_stride_row + s * weight_stride_s] with row = weight_rows ? weight_rows[q] : q, as uint8
 * (weight_kind 1, non-zero = 1) or float64 (weight_kind 2); it multiplies the 3x4 DLT term, so it enters squared.
 * zero_masked: an observation of weight 0 is read as (0,0) (local_refinement_tri).
 * out_points (n,3): eigenvector of the smallest eigenvalue of the 4x4 normal matrix over its last component; NaN when
 * fewer than two views have non-zero weight.  out_invalid_cheirality (n) or NULL: z <= 0 in ANY of the S views (1 for
 * the NaN points).  angle_mode 0: no angles.  1: out_max_angle (n) = largest triangulation angle in degrees over all
 * S x S camera pairs (0 for a non-finite point) and, when out_angle_flag is not NULL, out_angle_flag (n) =
 * that angle >= min_tri_angle.  2: out_angle_flag only, the pair scan stops at the first pair that passes.
 * workspace: vggx_multiview_workspace_bytes(cam_groups, S), read and written when angle_mode != 0. */
int vggx_multiview_triangulate(const double* cams, long cam_groups, int group_div, const void* tracks, int tracks_are_f64,
                               long track_stride_q, long track_stride_s, const void* weights, int weight_kind,
                               long weight_stride_row, long weight_stride_s, const int64_t* weight_rows, long n, int S,
                               int zero_masked, int angle_mode, double min_tri_angle, double* out_points,
                               uint8_t* out_invalid_cheirality, double* out_max_angle, uint8_t* out_angle_flag,
                               void* workspace, void* stream);

/* the reduced angle pass of vggx_multiview_triangulate alone, on given points (n,3); angle_mode 1 or 2 */
int vggx_max_tri_angle(const double* cams, long cam_groups, int group_div, const double* points, long n, int S,
                       int angle_mode, double min_tri_angle, double* out_max_angle, uint8_t* out_angle_flag,
                       void* workspace, void* stream);

/* calculate_triangulation_angle_batched: out (B,S*S), out[b][i*S+j] = angle in degrees at points[b] between cameras i
 * and j of group b (of the one shared set when cam_groups == 1, else cam_groups == B).  `denominator <= eps` -> 0. */
int vggx_tri_angle_table(const double* cams, long cam_groups, const double* points, long B, int S, double eps,
                         double* out, void* workspace, void* stream);

/* calculate_triangulation_angle: center1, center2 (K,3), points (P,3) -> out (K,P) degrees */
int vggx_tri_angle_pairs(const double* center1, const double* center2, long K, const double* points, long P, double eps,
                         double* out, void* stream);

/* calculate_normalized_angular_error_batched: point2D (B,N,2), point3D (P,N,3), cams (B,3,4) ->
 * out_angle (P,B,N) (radians, degrees with to_degree) and out_cos (P,B,N), the cosine clamped to [-1,1] */
int vggx_angular_error(const double* point2D, const double* point3D, const double* cams, long B, long N, long P,
                       int to_degree, double* out_angle, double* out_cos, void* stream);

#ifdef __cplusplus
}
#endif
#endif
