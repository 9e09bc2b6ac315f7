/*
 * vggsfm_amd -- EPnP and the local optimisation of the P3P RANSAC (fourth header of libvggsfm_amd.so).
 *
 *   efficient_pnp             vggsfm/two_view_geo/perspective_n_points.py:36-437
 *   the LO step of COLMAP's absolute pose LO-RANSAC (P3P minimal samples, EPnP on the inliers), applied to the final
 *   model of each virtual frame of vgg_p3p_ransac
 *
 * Conventions of include/vggsfm_amd.h hold: device pointers, `stream` a hipStream_t as void*, asynchronous, no
 * allocation, VGG_OK (0) or a negative VGG_ERR_* code.  The names carry the prefix vggp_; their rows in
 * vggsfm_amd/_lib.py stand under this header's key of HEADERS.
 * All arithmetic is float64 without floating-point contraction, no transcendental functions, every sum in a fixed
 * order, no atomics: a result is a function of its own problem alone, whatever else is in the launch.  One workgroup of
 * 256 threads per problem.
 *
 * Every entry checks its sizes before it launches: a negative count or fewer points than it needs (4 for the solver and
 * the local optimisation, 1 for the scoring), or NULL where data is required, is VGG_ERR_INVALID_ARGUMENT; more problems
 * than a grid dimension holds (2^31 - 1) is VGG_ERR_UNSUPPORTED; a count of 0 problems is a no-op that returns VGG_OK.
 */
#ifndef VGGSFM_AMD_PNP_H
#define VGGSFM_AMD_PNP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* efficient_pnp for num_problems problems: y = Proj(x R + T) in the reference's row-vector convention.
 * x (num_problems,num_points,3), or (num_points,3) shared by all problems when x_shared != 0; y
 * (num_problems,num_points,2) normalised image coordinates; weight (num_problems,num_points) a mask (0 = the point
 * enters no sum: whatever its slots of x and y hold, NaN included, never reaches a result) or NULL = all points.
 * skip_quadratic != 0: only the eigenvector of the smallest eigenvalue is a candidate.
 * out_R (num_problems,9) row-major, out_T (num_problems,3), out_err_2d, out_err_3d (num_problems), out_x_cam
 * (num_problems,num_points,3) or NULL (the slots of masked-out points are set to 0), out_variant (num_problems): the
 * candidate that won, 0 = the kernel vector alone, 1..3 = cases 1..3 (the first minimum of err_2d), out_valid
 * (num_problems).  A problem with fewer than 4 weighted points, or with a candidate that is not finite, gets valid 0,
 * R = identity, T = 0, x_cam = 0, variant 0 and both errors +infinity. */
int vggp_epnp_solve(const double* x, int x_shared, const double* y, const uint8_t* weight, long num_problems,
                    int num_points, int skip_quadratic, double* out_R, double* out_T, double* out_err_2d,
                    double* out_err_3d, double* out_x_cam, int32_t* out_variant, uint8_t* out_valid, void* stream);

/* support of given poses under the rule of vgg_p3p_ransac: poses (num_frames,num_poses,12) as [R|t] row-major,
 * points2D_normalized (num_frames,num_points,2), points3D (num_points,3), candidate_mask (num_frames,num_points) or NULL,
 * max_error_sq (num_frames) device memory.  A match is an inlier when it is a candidate, its depth is positive and its
 * squared residual on the normalised plane is <= max_error_sq[frame].  out_counts, out_residual_sums
 * (num_frames,num_poses), out_masks (num_frames,num_poses,num_points) or NULL. */
int vggp_pose_score(const double* poses, const double* points2D_normalized, const double* points3D,
                    const uint8_t* candidate_mask, const double* max_error_sq, long num_frames, int num_poses,
                    int num_points, int32_t* out_counts, double* out_residual_sums, uint8_t* out_masks, void* stream);

/* local optimisation of one pose per (virtual) frame, in place: pose (num_frames,12), num_inliers (num_frames),
 * residual_sum (num_frames), inlier_mask (num_frames,num_points); the other inputs as for vggp_pose_score.
 * A frame whose num_inliers is <= 0 on entry ("nothing found") is left untouched.  Otherwise round 0 recomputes the
 * support of the incoming pose (the incoming sums and mask are not trusted); then up to max_rounds times: stop with
 * fewer than 6 inliers; EPnP on the inliers; score the new pose against all candidates; keep it when it has more
 * inliers, or as many and a smaller residual sum; stop otherwise (also when EPnP flags the problem invalid).
 * max_rounds = 0 leaves the pose bit for bit and stores its recomputed support. */
int vggp_epnp_lo(const double* points2D_normalized, const double* points3D, const uint8_t* candidate_mask,
                 const double* max_error_sq, long num_frames, int num_points, int max_rounds, double* pose,
                 int32_t* num_inliers, double* residual_sum, uint8_t* inlier_mask, void* stream);

#ifdef __cplusplus
}
#endif
#endif
