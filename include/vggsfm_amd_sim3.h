/*
 * vggsfm_amd -- Sim(3) alignment and all-pairs pose errors (sixth header of libvggsfm_amd.so).
 *
 *   weighted Umeyama, hypothesis scoring and a 3-point LO-RANSAC over 3D-3D correspondences (what pycolmap users reach
 *   through estimate_sim3d[_robust] and align_reconstructions_via_*), and the pair errors of vggsfm/utils/metric.py
 *   (camera_to_rel_deg: rotation_angle, translation_angle, compare_translation_by_angle).
 *
 * Conventions of include/vggsfm_amd.h hold: device pointers, `stream` a hipStream_t as void*, asynchronous (no entry
 * synchronises with the host), no allocation, VGG_OK (0) or a negative VGG_ERR_* code.  The names carry the prefix vggs_;
 * their rows in vggsfm_amd/_lib.py stand under this header's key of HEADERS.
 *
 * A transform is 13 doubles: s, R row-major (9), t (3), with  tgt ~ s R src + t.  Point data is float64, masks are uint8.
 * All arithmetic is float64 without floating-point contraction; every sum is taken in a fixed order (block trees and
 * ordered second stages over per-workgroup partials in the workspace); there are no floating-point atomics.  Two runs
 * give the same bits, whatever the workspace held before: every entry writes all of the workspace it later reads.
 *
 * Every entry checks its sizes before it launches: a negative count or NULL where data is required is
 * VGG_ERR_INVALID_ARGUMENT; a workspace smaller than vggs_sim3_workspace_bytes is VGG_ERR_WORKSPACE; more problems than a
 * grid dimension holds (65535) is VGG_ERR_UNSUPPORTED; num_problems, num_points or num_hypotheses equal to 0 is a no-op
 * that returns VGG_OK.
 */
#ifndef VGGSFM_AMD_SIM3_H
#define VGGSFM_AMD_SIM3_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of workspace that every vggs_sim3_* entry accepts for these sizes (num_hypotheses may be 0 for the fit alone) */
size_t vggs_sim3_workspace_bytes(int num_problems, int num_points, int num_hypotheses);

/* weighted Umeyama: src, tgt (num_problems,num_points,3); weights (num_problems,num_points) doubles >= 0 or NULL (all
 * ones); a point of weight 0 (or of a weight that is not > 0) is not read.  Weighted means first, then the centred
 * moments Sigma = (1/W) sum w (tgt - mu_t)(src - mu_s)^T and sigma^2 = (1/W) sum w |src - mu_s|^2; R from Sigma with
 * det R = +1; s = trace(D S) / sigma^2, or 1 when estimate_scale == 0; t = mu_t - s R mu_s.
 * out_transform (num_problems,13), out_valid (num_problems).  valid = 0 with the identity transform: fewer than 3
 * points of positive weight, sigma^2 = 0, a collinear weighted source set (second eigenvalue of its 3x3 scatter
 * <= 1e-12 x the first), or a result that is not finite or has s <= 0.  A planar set is valid. */
int vggs_sim3_fit(const double* src, const double* tgt, const double* weights, int num_problems, int num_points,
                  int estimate_scale, double* out_transform, uint8_t* out_valid, void* workspace, size_t workspace_bytes,
                  void* stream);

/* support of given transforms: transforms (num_problems,num_hypotheses,13), valid (num_problems,num_hypotheses), mask
 * (num_problems,num_points) or NULL (a point of mask 0 is not read), max_error (num_problems) in target units.  A point
 * is an inlier when |tgt - (s R src + t)|^2 <= max_error^2.  out_counts (num_problems,num_hypotheses), -1 for an invalid
 * hypothesis; out_residual_sums (num_problems,num_hypotheses): the squared residuals of the inliers, 0 when invalid. */
int vggs_sim3_score(const double* src, const double* tgt, const uint8_t* mask, const double* transforms,
                    const uint8_t* valid, const double* max_error, int num_problems, int num_points, int num_hypotheses,
                    int32_t* out_counts, double* out_residual_sums, void* workspace, size_t workspace_bytes, void* stream);

/* LO-RANSAC: samples (num_problems,num_hypotheses,3) point indices.  A sample is invalid when an index repeats, is out
 * of range or masked out, or its fit is invalid.  All hypotheses are scored; the winner has the most inliers, then the
 * smaller inlier residual sum, then the lower index.  Then up to lo_rounds times: fit on the inliers of the current best,
 * score the result, accept it only if it ranks strictly better; stop when it is not accepted, when its fit is invalid,
 * or when an accepted round left the inlier set unchanged.  lo_rounds = 0 returns the minimal winner as it is.
 * out_transform (num_problems,13), out_num_inliers (num_problems), out_inlier_mask (num_problems,num_points),
 * out_residual_sum (num_problems), out_best_index (num_problems; -1: no valid hypothesis), out_lo_accepted
 * (num_problems), out_success (num_problems): 0 when no hypothesis was valid or the result has fewer than min_inliers
 * (>= 3) inliers; then the identity, an all-zero mask, count 0 and sum 0 are written.  out_counts, out_residual_sums
 * (num_problems,num_hypotheses): the score table of the minimal hypotheses, both or neither may be NULL. */
int vggs_sim3_ransac(const double* src, const double* tgt, const uint8_t* mask, const double* max_error,
                     const int32_t* samples, int num_problems, int num_points, int num_hypotheses, int lo_rounds,
                     int min_inliers, int estimate_scale, double* out_transform, int32_t* out_num_inliers,
                     uint8_t* out_inlier_mask, double* out_residual_sum, int32_t* out_best_index, int32_t* out_lo_accepted,
                     uint8_t* out_success, int32_t* out_counts, double* out_residual_sums, void* workspace,
                     size_t workspace_bytes, void* stream);

/* all-pairs pose errors: pred, gt (num_cameras,3,4) world-to-camera [R|t] (x_cam = R X + t); for the
 * num_cameras (num_cameras - 1) / 2 pairs i < j in the order of torch.combinations, with the relative pose
 * R_ij = R_j R_i^T, t_ij = t_j - R_ij t_i of each set:
 *   out_rot_deg:   arccos(1 - 2 max(1 - d2, 1e-15)), d2 = (1 + trace(R_ij,gt^T R_ij,pred)) / 4  (the squared quaternion
 *                  product of rotation_angle), in degrees;
 *   out_trans_deg: compare_translation_by_angle of the two t_ij (unit vectors by |t| + 1e-15, arccos(sqrt(1 - max(1 -
 *                  dot^2, 1e-15))), 1e6 when not finite) in degrees, then min(a, |180 - a|) (ambiguity=True).
 * One thread per pair.  Fewer than 2 cameras is a no-op. */
int vggs_pose_pair_errors(const double* pred, const double* gt, int num_cameras, double* out_rot_deg,
                          double* out_trans_deg, void* stream);

#ifdef __cplusplus
}
#endif
#endif
