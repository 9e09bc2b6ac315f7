/*
 * vggsfm_amd -- covariance of a bundle adjustment (fifth header of libvggsfm_amd.so).
 *
 *   the uncertainty of poses, intrinsics and points at the current state of a vgg_ba_problem: (J^T J)^-1 over the active
 *   columns, what Ceres' Covariance and COLMAP's bundle-adjustment covariance estimator offer [EXT: both are third-party,
 *   absent from the reference tree -- no parity is claimed].  DESIGN.md section 19.
 *
 * Conventions of include/vggsfm_amd.h hold: device pointers, `stream` a hipStream_t as void*, no allocation, VGG_OK (0) or a
 * negative VGG_ERR_* code.  The names carry the prefix vggc_; their rows in vggsfm_amd/_lib.py stand under this
 * header's key of HEADERS.  All arithmetic is float64 without
 * floating-point contraction, every sum in a fixed order, no atomics: two calls on the same input give the same bits.
 * Every entry checks its sizes before it launches: a negative size, or NULL where data is required, is
 * VGG_ERR_INVALID_ARGUMENT; a size beyond what the index arithmetic holds is VGG_ERR_UNSUPPORTED; a workspace that is too
 * small is VGG_ERR_WORKSPACE; a count of 0 is a no-op that returns VGG_OK.
 * vggc_spd_inverse is asynchronous.  vggc_ba_covariance synchronises the stream ONCE, at its start, where vgg_ba_begin does
 * (it reads the tile table, a few KB); everything behind that is enqueued.
 */
#ifndef VGGSFM_AMD_COVARIANCE_H
#define VGGSFM_AMD_COVARIANCE_H
#include <stddef.h>
#include <stdint.h>

#include "vggsfm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Inverse of a symmetric positive-definite matrix, in place.  A (n,n) row-major; only its lower triangle is read.  A is
 * overwritten by the full inverse: the lower triangle is computed, the upper triangle is a copy of it, so the result is
 * bitwise symmetric.  n need not be a multiple of anything.
 * Steps: a copy of the lower triangle in the workspace is factored by vgg_cholesky_solve (with a zero right-hand side behind
 * it, where the single-launch factorisation wants it); the 64 x 64 diagonal blocks of the factor L are inverted; the block
 * columns of L^-1 follow as independent forward substitutions in 64-column blocks; A^-1 = L^-T L^-1.  The block products run
 * on the FP64 matrix cores.  Nothing of what the factorisation leaves in the strict upper triangle, in its own workspace or
 * in any padding is read.
 * *device_fail (int32, device, zeroed by the caller) is set non-zero by the factorisation on a non-positive pivot, as
 * vgg_cholesky_solve sets it; the output is then all NaN.  No kernel of this entry waits for another: nothing spins or times
 * out beyond what vgg_cholesky_solve itself does.
 * workspace: vggc_spd_inverse_workspace_bytes(n) device bytes, 256-byte aligned (0 for n <= 0).  n <= 46340 - 64. */
size_t vggc_spd_inverse_workspace_bytes(int n);
int vggc_spd_inverse(double* A, int n, void* workspace, int32_t* device_fail, void* stream);

/* What vggc_ba_covariance computes (`flags`, at least one): */
#define VGGC_COV_CAMERAS 1   /* out_reduced, out_pose, out_intr, out_pose_intr: those that are not NULL */
#define VGGC_COV_POINTS 2    /* out_points (required then) */

/* Covariance (J^T J)^-1 at the problem's current state over its active columns.  J is the robustified Jacobian the solver
 * linearises with (csrc/camera_model.hpp: the loss corrector included), unscaled and undamped.  It is taken in the solver's
 * TANGENT: per camera the rotation as Ceres' quaternion plus q <- exp(d) (x) q with exp(d) = [sin|d| / |d| d, cos|d|] -- d is
 * HALF the rotation vector --, then the translation; then the refined intrinsics (f, k: those that refine_focal /
 * refine_extra select).  The rotation block is therefore in half-angle units: the covariance of the rotation VECTOR is four
 * times that block, its cross terms with anything else twice.  No variance factor is applied (unit weights).
 *   n = 6 num_cams + kd num_intr, kd = refined intrinsics per block (0..2); the reduced system's column order:
 *   camera c at 6 c .. 6 c + 5, intrinsics block a at 6 num_cams + kd a ..
 *   out_reduced    (n, n)               the camera and intrinsics columns, both triangles
 *   out_pose       (num_cams, 6, 6)     diagonal blocks of it
 *   out_intr       (num_intr, kd, kd)
 *   out_pose_intr  (num_cams, 6, kd)    camera c against its own (or the shared) intrinsics block
 *   out_points     (num_pts, 3, 3)      Sigma_pp = V^-1 + G Sigma_uu G^T, V = sum E^T E, G = V^-1 W^T over the columns u of the
 *                                       cameras that observe the point and their (or the shared) intrinsics
 * Each output may be NULL (out_points not with VGGC_COV_POINTS); none needs another.  With kd = 0 out_intr and out_pose_intr
 * are not touched.  Constant and unobserved columns -- and constant or unobserved points -- have zero variance and zero
 * cross terms.  The state (cam_q, cam_t, intr, pts) is read, never written.
 * The reduced system comes from the solver's own launches (vgg_ba_begin, rank 0 of 1, and vgg_ba_phase 1 on a private part of
 * the workspace) with a copy of `options` whose trust-region radius is 2^900 and whose overlap_factorization is 0: the LM
 * damping clip(colsq s^2, min_lm_diagonal, max_lm_diagonal) / radius is then at most 2^-900 of a scaled diagonal element of
 * at least min_lm_diagonal and is lost in the first addition.  The Jacobi scaling is undone with the
 * solver's own scales (vgg_ba_reduce_buffer, which = 8), the system inverted densely by vggc_spd_inverse.
 * *device_fail (int32, device, zeroed by the caller): non-zero when the reduced system or a point block is not positive
 * definite -- typically a gauge that is not fixed; the outputs are then NaN where they depend on it.
 * workspace: vggc_ba_covariance_workspace_bytes(problem, options, flags) device bytes, 256-byte aligned.  Its head is the
 * solver's workspace: after the call vgg_ba_reduce_buffer(problem, options, workspace, 0, ..) addresses U, g and the per-camera
 * costs at the state (the cost is half their sum). */
size_t vggc_ba_covariance_workspace_bytes(const vgg_ba_problem* problem, const vgg_ba_options* options, int flags);
int vggc_ba_covariance(const vgg_ba_problem* problem, const vgg_ba_options* options, void* workspace, size_t workspace_bytes,
                       int flags, double* out_reduced, double* out_pose, double* out_intr, double* out_pose_intr,
                       double* out_points, int32_t* device_fail, void* stream);

#ifdef __cplusplus
}
#endif
#endif
