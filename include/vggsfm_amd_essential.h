/*
 * vggsfm_amd -- essential matrices by the 5-point algorithm with LO-RANSAC (third header of libvggsfm_amd.so).
 *
 *   estimate_essential        vggsfm/two_view_geo/essential.py:111-200
 *   run_5point                vggsfm/two_view_geo/essential.py:203-264
 *   null_to_Nister_solution   vggsfm/two_view_geo/essential.py:271-488
 *
 * Conventions of include/vggsfm_amd.h hold: device pointers, `stream` a hipStream_t as void*, asynchronous, no
 * allocation, VGG_OK (0) or a negative VGG_ERR_* code.  The names carry the prefix vgge_emat_; their rows in
 * vggsfm_amd/_lib.py stand under this header's key of HEADERS.
 * All arithmetic is float64 without floating-point contraction, no transcendental functions, every sum in a fixed
 * order: a result is a function of its own (pair, sample) alone, whatever else is in the launch.
 *
 * Points are NORMALISED image coordinates (pixel - principal point) / focal length, (num_pairs, num_points, 2).
 * A 5-point solve gives ten candidate slots of 9 doubles (3x3 row-major, unit Frobenius norm, p2^T E p1 = 0) and ten
 * flags; the real roots of the degree-10 polynomial fill the first slots in ascending order, the other slots hold zeros
 * and flag 0.  A slot is also flagged 0 when a pivot of the elimination is zero or its matrix is not finite.  The real
 * roots are counted with a Sturm chain whose remainders are taken to lose exactly one degree each; a polynomial for which
 * one does not (a vanishing leading coefficient, a repeated root: a set of measure zero) gives a non-finite chain, the
 * count is then zero and ALL ten slots of that solve are flagged 0, its real roots included.
 */
#ifndef VGGSFM_AMD_ESSENTIAL_H
#define VGGSFM_AMD_ESSENTIAL_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* minimal solver: samples (num_samples,5) indices into the points, shared by all pairs -> out_emat
 * (num_pairs,num_samples,10,9), out_valid (num_pairs,num_samples,10).  A sample with an index outside
 * [0, num_points) is flagged 0 in all its slots and its points are not read. */
int vgge_emat_five_point(const double* points1, const double* points2, const int32_t* samples, int num_pairs,
                         int num_points, int num_samples, double* out_emat, uint8_t* out_valid, void* stream);

/* the same solve on the 9x9 matrix X^T X summed over ALL num_points rows of a set (run_5point with more than five
 * points); row_weights (num_sets,num_points) or NULL multiplies the rows of X.  out_emat (num_sets,10,9), out_valid
 * (num_sets,10) */
int vgge_emat_solve(const double* points1, const double* points2, const double* row_weights, long num_sets,
                    int num_points, double* out_emat, uint8_t* out_valid, void* stream);

/* inlier count and inlier residual sum (squared Sampson distance <= max_error_sq[pair]) of num_hypotheses matrices per
 * pair: emat (num_pairs,num_hypotheses,9), emat_valid (num_pairs,num_hypotheses); a hypothesis flagged 0 gets count -1
 * and sum 0.  max_error_sq (num_pairs) is device memory. */
int vgge_emat_score(const double* points1, const double* points2, const double* emat, const uint8_t* emat_valid,
                    const double* max_error_sq, int num_pairs, int num_points, int num_hypotheses, int32_t* out_counts,
                    double* out_residual_sums, void* stream);

/* local optimisation: for l < num_selected the inliers of hypothesis selected[pair][l] of src_emat
 * (num_pairs,num_src,9) are recomputed (src_counts (num_pairs,num_src): < 0 = not a hypothesis), X^T X is summed over
 * them and solved -> out_emat (num_pairs,num_selected,10,9), out_valid (num_pairs,num_selected,10).  Fewer than five
 * inliers, or a selected index outside [0, num_src): all ten slots flagged 0. */
int vgge_emat_refine(const double* points1, const double* points2, const double* src_emat, const int32_t* src_counts,
                     const int32_t* selected, const double* max_error_sq, int num_pairs, int num_points, int num_src,
                     int num_selected, double* out_emat, uint8_t* out_valid, void* stream);

#ifdef __cplusplus
}
#endif
#endif
