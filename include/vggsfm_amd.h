/*
 * vggsfm_amd -- C-ABI of the MI355X (gfx950) geometry hot path of VGGSfM.
 *
 * This is the drop-in boundary: plain pointers + sizes, no torch / pycolmap types.  Every pointer
 * named *device* is HBM memory of the current HIP device; `stream` is a hipStream_t passed as void*.
 * All entry points are asynchronous on `stream` unless stated, never allocate, and return VGG_OK (0)
 * or a negative VGG_ERR_* code.  Each one names the reference interface it replaces (paths under
 * /root/reference); the Python host side in vggsfm_amd/ mirrors the reference signatures on top.
 *
 * Layout conventions (the reference's own): extrinsics (S,3,4) row-major
 * [R|t] with x_cam = R X + t (OpenCV frame); intrinsics (S,3,3) row-major; tracks (S,P,2) pixels
 * (float32 as produced by the tracker, or float64); masks uint8 0/1; all geometry float64.
 */
#ifndef VGGSFM_AMD_H
#define VGGSFM_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VGG_OK 0
#define VGG_ERR_INVALID_ARGUMENT (-1)
#define VGG_ERR_HIP (-2)
#define VGG_ERR_WORKSPACE (-3)
#define VGG_ERR_UNSUPPORTED (-4)

/* library / build identification ("gfx950"), for loud failure when the wrong object is loaded */
const char* vgg_build_arch(void);
int vgg_abi_version(void);          /* VGG_ABI_VERSION of the build: bumped whenever a struct below changes layout */
#define VGG_ABI_VERSION 2
/* sizeof of the by-pointer structs as the library was compiled (which: 0 vgg_ba_problem, 1 vgg_ba_options,
 * 2 vgg_ba_iteration, 3 vgg_ba_summary; 0 for anything else): a binding checks its own layout against these and
 * refuses to drive a library built from another revision of this header (vggsfm_amd/_lib.py does). */
size_t vgg_abi_sizeof(int which);

/* ------------------------------------------------------------------------------------------
 * project_3D_points + img_from_cam       vggsfm/utils/triangulation_helpers.py:311-395
 * out_uv (S,P,2) and/or out_cam (S,3,P) may be NULL; intrinsics NULL == only_points_cam.
 * num_extra in {0,1,2,4} (SIMPLE_RADIAL / RADIAL / OPENCV distortion, distortion.py:102-159). */
int vgg_project_points(const double* points3D, int P, const double* extrinsics, const double* intrinsics,
                       const double* extra_params, int num_extra, int S, double* out_uv, double* out_cam,
                       void* stream);

/* filter_all_points3D(_single_chunk)      vggsfm/utils/triangulation_helpers.py:133-307
 * reprojection error^2 <= max^2 with depth > 0 (else `behind_value`: 1e6 there, 1e9 in refine_pose,
 * triangulation.py:308-312), >= 2 inlier views, |X| <= hard_max (<=0 disables), optional "some inlier
 * pair subtends >= min_tri_angle degrees".  out_mask (P); out_detail (S,P) or NULL.
 * workspace: vgg_filter_points_workspace_bytes(S) device bytes (only read when check_triangle). */
size_t vgg_filter_points_workspace_bytes(int S);
int vgg_filter_points(const double* points3D, int P, const void* tracks, int tracks_are_f64, const double* extrinsics,
                      const double* intrinsics, const double* extra_params, int num_extra, int S,
                      double max_reproj_error, double min_tri_angle, int check_triangle, double hard_max,
                      double behind_value, uint8_t* out_mask, uint8_t* out_detail, void* workspace, void* stream);

/* cam_from_img + iterative_undistortion   vggsfm/utils/triangulation_helpers.py:398-428,
 *                                         vggsfm/utils/distortion.py:27-99
 * out (S,P,2) f64.  With num_extra > 0 runs the reference's Newton iteration incl. its tensor-global
 * stopping rule; this SYNCHRONISES the stream every 8 iterations; *iterations_run (host) may be NULL. */
size_t vgg_cam_from_img_workspace_bytes(int S, int P, int max_iterations);
int vgg_cam_from_img(const void* tracks, int tracks_are_f64, const double* intrinsics, const double* extra_params,
                     int num_extra, int S, int P, double* out, int max_iterations, double max_step_norm,
                     double rel_step_size, double eps, void* workspace, int* iterations_run, void* stream);

/* ------------------------------------------------------------------------------------------
 * triangulate_tracks_single_chunk         vggsfm/utils/triangulation.py:776-956
 * LO-RANSAC multi-view DLT for the N tracks of one chunk, one wavefront per track.
 *   tracks_t (N,S,2) f64: normalised rays, TRACK-major (the reference transposes too, :798)
 *   invalid_vis_conf_t (N,S) uint8 = (vis <= 0.05) | (score <= 0.5)              (:867-874)
 *   pairs (H,2) int32 device: hypothesis view pairs; the caller reproduces the reference's host-side
 *   torch.randperm draw (:804-813).  H <= 256, lo_num <= 64 (second round: min(10, lo_num), :902-904).
 * Hypotheses are ranked by inlier count in STABLE descending order (tie-break contract).
 * *threshold_io (host, in/out): calculate_residual_indicator (vggsfm/two_view_geo/utils.py:63-87)
 * normalises by the chunk-global max mean inlier error + 1e-6.  Pass 2*pi + 1e-6 (exact whenever some
 * hypothesis of the chunk has no inlier); on return it holds the measured value -- if it differs,
 * call again with the returned value.  Synchronises the stream once.
 * Outputs: points (N,3) f64, inlier_num (N) int64, inlier_mask (N,S) uint8. */
/* triangulate_tracks over ALL reference chunks of a call in one launch (vggsfm/utils/triangulation.py:712-758 splits
 * the track axis into ceil(S*N/819200) chunks, each with its own torch.randperm draw and its own chunk-global
 * residual-indicator threshold).  pairs [num_chunks,H,2] int32: the hypothesis pairs of every chunk, drawn by the
 * caller in chunk order; chunk c = tracks [c*chunk_size, min(N,(c+1)*chunk_size)).  thresholds_io: host array
 * [num_chunks], semantics of threshold_io above, per chunk.  One stream synchronisation.
 * Limits (both entries): 1 <= H <= 256 hypotheses per track, 1 <= lo_num <= 64 local-optimisation candidates;
 * VGG_ERR_INVALID_ARGUMENT beyond (the reference calls with H = 256 or 128 and lo_num = 50). */
size_t vgg_triangulate_chunks_workspace_bytes(int S, int num_chunks);
int vgg_triangulate_tracks_chunks(const double* extrinsics, const double* tracks_t, const uint8_t* invalid_vis_conf_t,
                                  const int32_t* pairs, int S, int N, int H, int num_chunks, int chunk_size, int lo_num,
                                  double max_angular_error_deg, double min_tri_angle_deg, double* out_points,
                                  int64_t* out_inlier_num, uint8_t* out_inlier_mask, double* thresholds_io,
                                  void* workspace, void* stream);
/* Asynchronous form of the same launch (round 4): nothing is copied back, nothing is waited for.  `num_chunks` consecutive
 * chunks starting at tracks_t[0]; thresholds_dev [num_chunks] and gmax_dev [num_chunks] (zeroed by the caller) are DEVICE
 * arrays -- gmax_dev receives the bit pattern of the largest mean inlier error of every chunk (compare with the threshold
 * semantics above); centers_dev [S][3] is scratch.  Lets the caller enqueue a call group of chunks by group of chunks while
 * it is still drawing the later groups' hypothesis pairs on the host. */
int vgg_triangulate_tracks_chunks_enqueue(const double* extrinsics, const double* tracks_t, const uint8_t* invalid_vis_conf_t,
                                          const int32_t* pairs, int S, int N, int H, int num_chunks, int chunk_size, int lo_num,
                                          double max_angular_error_deg, double min_tri_angle_deg, double* out_points,
                                          int64_t* out_inlier_num, uint8_t* out_inlier_mask, const double* thresholds_dev,
                                          unsigned long long* gmax_dev, double* centers_dev, void* stream);

/* triangulate_by_pair (vggsfm/utils/triangulation.py:45-135): the S-1 two-view DLT point clouds between frame 0 and
 * every other frame.  extrinsics [S,3,4] f64, tracks_normalized [S,N,2] f64 (frame-major, camera rays) ->
 * out_points [S-1,N,3] f64.  Cheirality and triangulation angle are elementwise follow-ups on the host side. */
int vgg_triangulate_by_pair(const double* extrinsics, const double* tracks_normalized, int S, int N, double* out_points,
                            void* stream);

size_t vgg_triangulate_workspace_bytes(int S, int N, int H, int lo_num);
int vgg_triangulate_tracks(const double* extrinsics, const double* tracks_t, const uint8_t* invalid_vis_conf_t,
                           const int32_t* pairs, int S, int N, int H, int lo_num, double max_angular_error_deg,
                           double min_tri_angle_deg, double* out_points, int64_t* out_inlier_num,
                           uint8_t* out_inlier_mask, double* threshold_io, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------
 * Bundle adjustment / pose refinement = what the reference obtains from
 *   pycolmap.bundle_adjustment   vggsfm/utils/triangulation.py:213,1050,1142; runners/video_runner.py:508
 *   pycolmap.pose_refinement     vggsfm/utils/triangulation.py:387,590; runners/video_runner.py:1001
 * (COLMAP BundleAdjuster on Ceres' Levenberg-Marquardt, Schur elimination of the points).
 *
 * State and structure live on the device in flat arrays; nothing is marshalled through host objects.
 * Observations are given twice: point-major CSR (row_ptr/obs_*) and camera-major CSR (col_ptr/cobs_*),
 * both sorted ascending in the minor index.  `tile_*` is the block-sparse Schur work list built by the
 * host side (vggsfm_amd/ba.py: build_schur_tiles): cameras are grouped 16 at a time, a "segment" is the
 * run of one point's observations inside one camera group, an "entry" pairs two segments of one point. */
typedef struct {
  int32_t num_cams, num_pts, num_obs, num_intr;   /* num_intr == 1 (shared camera) or == num_cams */
  int32_t camera_model;                           /* 0 SIMPLE_PINHOLE  1 SIMPLE_RADIAL */
  int32_t refine_focal, refine_extra;             /* principal point is always constant */
  int32_t loss;                                   /* 0 trivial 1 Cauchy 2 Huber 3 SoftL1 */
  double loss_scale;
  /* state, in/out (device) */
  double* cam_q;              /* [num_cams,4] unit quaternion x,y,z,w */
  double* cam_t;              /* [num_cams,3] */
  double* intr;               /* [num_intr,4] f,cx,cy,k */
  double* pts;                /* [num_pts,3] */
  /* structure (device) */
  const int32_t* row_ptr;     /* [num_pts+1] */
  const int32_t* obs_cam;     /* [num_obs] */
  const float* obs_uv;        /* [num_obs,2] */
  const int32_t* col_ptr;     /* [num_cams+1] */
  const int32_t* cobs_pt;     /* [num_obs] */
  const float* cobs_uv;       /* [num_obs,2] */
  const uint8_t* cam_const;   /* [num_cams] bit0: pose constant; bit1..3: t_x,t_y,t_z constant; or NULL */
  const uint8_t* intr_const;  /* [num_intr] or NULL */
  const uint8_t* pt_const;    /* [num_pts] or NULL */
  /* Schur tile work list (device) */
  int32_t num_chunks;
  int32_t num_tile_batches;   /* >= 1: the tiles are cut into batches of consecutive camera groups groupI (tile_batches) */
  const int32_t* chunk_desc;  /* [num_chunks,6] = groupI, groupJ, tile_entry_begin, tile_entry_end, j, J:
                                 workgroup j of the J of its tile takes the 32-entry sub-chunks j, j+J, ... */
  const int32_t* entries;     /* [num_entries,4] = point index (row of pts), segment_A, segment_B, maskA | maskB<<16 of the
                                 QUAD: the four consecutive entries, aligned to tile_entry_begin, that the kernel packs
                                 along K (bit l of a mask: camera group*16+l observes one of the four points; 16-row
                                 blocks of the tile without any camera are skipped for the quad) */
  int32_t num_segments;       /* segments: runs of one point's observations inside one camera group */
  const int32_t* obs_slot;    /* [num_obs] = segment*16 + (camera % 16): where the point-major observation's
                                 Schur factor lives in the zero-padded segment buffer */
  int32_t num_tiles;
  const int32_t* tile_desc;   /* [num_tiles,4] = groupI, groupJ, chunk_begin, chunk_end (chunks of one tile
                                 are consecutive; their partial sums are reduced in this order) */
  const int32_t* tile_batches;/* HOST array [num_tile_batches,6] = chunk_begin, first_diagonal_chunk, chunk_end, tile_begin,
                                 tile_end, first_camera_group.  Batch-major order of chunk_desc / tile_desc: inside a batch
                                 the chunks of the off-diagonal tiles (groupI < groupJ) come first, then the diagonal
                                 ones (separate launches).  Column block g of the reduced system only receives sums
                                 from tiles with groupI <= g: it is complete once the batches up to that of group g
                                 are done, so the factorisation can start while later batches are being computed. */
  int32_t chol_split_a;       /* Block-diagonal leading part of the reduced camera system, 0 = none.  If the cameras are */
  int32_t chol_split_b;       /* ordered so that no point is seen both by one of the first chol_split_a / 6 cameras and by
                                 one of the next chol_split_b / 6 (sliding-window / video-like visibility: the host side
                                 checks this and orders the cameras, ba.py), the pose columns [0, a) and [a, a + b) of S
                                 do not couple and their factorisations advance side by side in shared launches
                                 (chol.hip); a must be a multiple of 64.  The caller guarantees the structure -- with
                                 several GPUs for the SUM over ranks. */
  const int32_t* chol_first_blk; /* device, optional: ROW ENVELOPE of the reduced system in 64-column blocks.  Entry r (r = 0 ..
                                 ceil(n / 64) - 1) = the first block column in which block row r (rows 64 r .. 64 r + 63 of S) can
                                 hold a non-zero; the Cholesky factor keeps the row envelope of the matrix, so the dataflow
                                 factorisation (chol.hip) skips the tiles left of it and drops their dependences: camera
                                 blocks that do not couple factor concurrently, whatever their number (ba.py:
                                 find_camera_order -- nested-dissection order of sliding-window / video visibility).  NULL =
                                 dense (then chol_split_a / b, if set, describe a two-block leading part).  The caller
                                 guarantees the structure, with several ranks for the SUM of their systems. */
  int32_t merged_tile_launch;    /* 1: the off-diagonal and the diagonal chunks of a batch run in ONE launch (the host sized them for
                                 one shared resident round) -- small problems, where the second launch costs more than the
                                 lower occupancy of the merged kernel */
} vgg_ba_problem;

typedef struct {
  int32_t max_num_iterations;
  int32_t max_num_consecutive_invalid_steps;
  int32_t jacobi_scaling;
  double function_tolerance, gradient_tolerance, parameter_tolerance;
  double initial_trust_region_radius, max_trust_region_radius, min_trust_region_radius;
  double min_lm_diagonal, max_lm_diagonal, min_relative_decrease;
  int32_t overlap_factorization; /* 0 = off; otherwise the number of CUs (a multiple of 32) given to the factorisation
                                    while it overlaps the tile batches 1.. (>= 2 batches; they then run on the other
                                    CUs, both on CU-masked side streams joined back into `stream`).  Single GPU only:
                                    the multi-GPU loop all-reduces the complete system between phases 1 and 2 */
} vgg_ba_options;

typedef struct {
  int32_t iteration;
  int32_t successful;
  double cost, cost_change, gradient_max_norm, step_norm, relative_decrease, radius;
} vgg_ba_iteration;

typedef struct {
  double initial_cost, final_cost;
  int32_t num_iterations, num_successful_steps, num_unsuccessful_steps;
  int32_t termination;        /* 0 iteration cap, 1 gradient, 2 function, 3 parameter, 4 radius, 5 failure */
  int32_t n_reduced, num_log;
} vgg_ba_summary;

/* device bytes vgg_ba_solve needs in `workspace` (256-byte aligned base) */
size_t vgg_ba_workspace_bytes(const vgg_ba_problem* problem, const vgg_ba_options* options);

/* Runs the whole LM loop on `stream` (device-side control flow: the host enqueues
 * max_num_iterations iterations, a device flag turns the rest into no-ops after termination),
 * then synchronises ONCE to copy summary + per-iteration log (log_cap entries, may be NULL). */
int vgg_ba_solve(const vgg_ba_problem* problem, const vgg_ba_options* options, void* workspace,
                 size_t workspace_bytes, vgg_ba_summary* summary, vgg_ba_iteration* log, int log_cap, void* stream);

/* Multi-GPU (points sharded across ranks, cameras replicated): the same loop split into phases so
 * that the host can interleave RCCL all-reduces on the same stream.
 *   vgg_ba_begin    : init control block; camera-side J^T J / J^T r / cost of the local points at the start point
 *                      -> reduce buffer 0
 *   phase 0 LINEARIZE: launches nothing: reduce buffer 0 holds the local camera-side terms of the current x    -> SUM
 *   phase 1 SCHUR    : point blocks, reduced camera system of the local points -> reduce buffer 1 (SUM),
 *                      gradient max of local points                            -> reduce buffer 2 (MAX)
 *                      (buffer 1 = S | rhs of  S y = rhs,  S = A_cc - sum_p W_p V_p^-1 W_p^T,  rhs = + J_c^T r - sum_p W_p V_p^-1
 *                      J_p^T r  in Jacobi-scaled columns, damping included, lower triangle; the step is -y o scale.  An inactive
 *                      column j -- constant, or of a frame without observations -- holds the damping of a zero column,
 *                      min_lm_diagonal / radius, at S[j][j] on rank 0 and zeros elsewhere in its row, its column and rhs[j];
 *                      phase 2 puts the unit diagonal there after the sum.  tests/test_gpu_ba_system.py)
 *   phase 2 STEP     : Cholesky + back-substitution, then the camera-side pass at the candidate: its local cost, the
 *                      model cost change and the step norms                    -> reduce buffer 3 (SUM); its local
 *                      J^T J / J^T r / cost are kept in the workspace (not a reduce buffer)
 *   phase 3 UPDATE   : trust-region decision, commit.  Accepted: the candidate's local terms of phase 2 are copied into
 *                      reduce buffer 0 (the next phase 0 needs no pass).  Rejected: buffer 0 keeps the all-reduced terms of
 *                      the current x on rank 0 and is cleared on the other ranks, so that the next SUM gives them back
 *   phase 4 / 5      : pack / unpack the lower triangle of the reduced system + rhs into / from reduce buffer 4
 *                      (n(n+1)/2 + n doubles): all-reducing buffer 4 between them replaces the all-reduce of
 *                      buffer 1 (n^2 + n doubles, strict upper triangle all zero: vgg_ba_begin clears it, no phase writes
 *                      it) at half the payload
 *   phase 6          : unpack from the OUTPUT of a reduce-scatter + all-gather of buffer 4, read in place: with W ranks
 *                      and c = ceil(count / W), phase 4 also zeroes buffer 4 up to W c doubles (it is carved with that
 *                      padding: the reduce-scatter input, no staging copy) and puts the rank's gradient maximum at
 *                      element c of buffer 5 (c + 1 doubles: reduce-scatter output = all-gather input); buffer 6
 *                      (W (c + 1) doubles) is the all-gather output; phase 6 rebuilds S | rhs from its W slices and
 *                      takes the maximum of the W riding gradient norms (replaces the MAX reduce of buffer 2).  W <= 1024
 *   phases 7..12     : the SPLIT exchange (round 6) -- phase 1 and the exchange of the system cut in two so that the first
 *                      half of the payload travels while the diagonal tile launch computes the second:
 *                      7 = phase 1 up to the sums of the OFF-DIAGONAL tiles; 8 = pack part A (the elements of the lower
 *                      triangle whose row and column belong to cameras of different 16-camera groups -- all the off-diagonal
 *                      launch fills) into buffer 4; 9 = the rest of phase 1 (diagonal launch, its sums, assemble); 10 = pack
 *                      part B (everything else + rhs) behind it; 11 = S | rhs from the two parts' all-gather outputs; 12 =
 *                      query, to be called ONCE per workspace before phases 7..11: VGG_OK if the split is available for this problem (one tile
 *                      batch, separate tile launches, more than 16 cameras) -- it then also writes the rows' offsets inside the two parts into the
 *                      workspace --, VGG_ERR_UNSUPPORTED otherwise (nothing is launched).  With a = vgg_ba_reduce_buffer(7) elements in
 *                      part A, b = count(4) - a, ca = ceil(a / W), cb = ceil(b / W): buffer 4 = [A: W ca | B: W cb] (reduce-
 *                      scatter inputs), buffer 5 = [A: ca | B: cb + 1] (the rank's slices; the gradient maximum rides behind
 *                      B's), buffer 6 = [A: W ca | B: W (cb + 1)] (all-gather outputs); buffers 4 and 6 are carved with the
 *                      padding both forms need up to W = 1024 (count(6) = count(4) + 3072)
 * vgg_ba_reduce_buffer returns the device address / element count (doubles) of each reduce buffer (which = 7: buffer 4's address
 * and the element count of part A; which = 8: no reduce buffer but the solver's own Jacobi scales of the n reduced columns,
 * 1 / (1 + sqrt(colsq)), or 1 without jacobi_scaling -- valid once phase 1 has run; include/vggsfm_amd_covariance.h undoes the
 * scaling of buffer 1 with them). */
int vgg_ba_begin(const vgg_ba_problem* problem, const vgg_ba_options* options, void* workspace, size_t workspace_bytes,
                 int rank, int world_size, void* stream);
int vgg_ba_phase(const vgg_ba_problem* problem, const vgg_ba_options* options, void* workspace, int phase,
                 void* stream);
int vgg_ba_reduce_buffer(const vgg_ba_problem* problem, const vgg_ba_options* options, void* workspace, int which,
                         double** device_ptr, size_t* count);
int vgg_ba_finish(const vgg_ba_problem* problem, const vgg_ba_options* options, void* workspace,
                  vgg_ba_summary* summary, vgg_ba_iteration* log, int log_cap, void* stream);
/* Has the solve terminated?  Copies the 4-byte device flag and synchronises the stream (what vgg_ba_solve does every
 * 8 iterations): a phase-driven caller uses it to stop enqueuing iterations -- and, with several ranks, their
 * collectives -- once the (rank-identical) device-side decision has ended the solve. */
int vgg_ba_poll_done(const vgg_ba_problem* problem, const vgg_ba_options* options, void* workspace, int32_t* done_host,
                     void* stream);

/* pycolmap.pose_refinement for a batch of frames   vggsfm/utils/triangulation.py:387,590 (loops :341-441, :542-608)
 * = COLMAP RefineAbsolutePose: points constant, robust loss (reference: Cauchy, scale 1), unknowns pose
 * (+ focal if refine_flags bit0, + extra param if bit1).  One workgroup solves one frame; frames are
 * independent.  frame_ids (F) int32 device: frames to refine; inlier_mask (S,P) uint8: observations used.
 * cam_q (S,4) / cam_t (S,3) / intr (S,4 = f,cx,cy,k PER FRAME) are updated in place for those frames.
 * options: Ceres defaults for this call site are max_num_iterations 100, function_tolerance 1e-6,
 * gradient_tolerance 1.0, parameter_tolerance 1e-8.  summaries (F) device or NULL. */
int vgg_pose_refine(const double* points3D, const void* tracks, int tracks_are_f64, const uint8_t* inlier_mask, int S,
                    int P, const int32_t* frame_ids, int num_frames, double* cam_q, double* cam_t, double* intr,
                    int camera_model, const uint8_t* refine_flags, const vgg_ba_options* options, int loss,
                    double loss_scale, vgg_ba_summary* summaries, void* stream);

/* pycolmap.absolute_pose_estimation, the RANSAC part   vggsfm/utils/triangulation.py:324-326,400-432 (fallback of
 * refine_pose), vggsfm/runners/video_runner.py:987-998 (align_next_window, use_pnp)
 * = COLMAP EstimateAbsolutePose restated (third-party, absent from the reference tree; PARITY UNPINNED, see
 * oracle/p3p.py): P3P minimal samples, squared reprojection error on the normalised image plane, points with
 * depth <= 0 never inliers, support = (most inliers, then smallest inlier residual sum, then lowest index).
 * Deviations: the caller draws a fixed number of samples (no adaptive trial count), no EPnP step inside the loop
 * (the local optimisation is a separate, opt-in entry applied to each frame's winner: vggsfm_amd_pnp.h);
 * the caller runs vgg_pose_refine on the returned inliers afterwards, as COLMAP does.
 * All num_frames (virtual) frames run concurrently.  A virtual frame is (frame, focal length factor): COLMAP's
 * estimate_focal_length runs one RANSAC per factor -- the caller passes the points normalised with each scaled
 * camera, frames_per_sample_set consecutive virtual frames share one sample set.
 *   points2D_normalized [num_frames][num_points][2] f64, points3D [num_points][3] f64,
 *   candidate_mask [num_frames][num_points] uint8 or NULL (matches that take part), samples
 *   [num_frames / frames_per_sample_set][num_hypotheses][3] int32 indices into num_points (distinct, candidates),
 *   max_error_sq [num_frames] f64 (squared threshold on the normalised plane = (max_error / focal)^2).
 * Outputs per virtual frame: out_pose [12] row-major [R|t] (zeros if nothing found), out_num_inliers (0 if nothing
 * found), out_residual_sum, out_best (hypothesis * 4 + solution, -1 if none), out_inlier_mask [num_points].
 * workspace: vgg_p3p_ransac_workspace_bytes(num_frames, num_hypotheses) bytes of device memory owned by the caller.
 * Two of its blocks are readable after the call (once the stream has been synchronised); with FH = num_frames *
 * num_hypotheses:
 *   hypotheses  [num_frames][num_hypotheses][4][12] f64 at byte 0: the up to four poses of every sample, row-major
 *               [R|t], zeros where the solution is not valid
 *   validity    [num_frames][num_hypotheses][4] uint8 (0 / 1) at byte FH * 432, the last block (after the hypotheses,
 *               FH * 4 f64 residual sums and FH * 4 int32 inlier counts, which are scratch)
 * out_best indexes the hypotheses of its frame as a flat [4 * num_hypotheses][12] array. */
size_t vgg_p3p_ransac_workspace_bytes(int num_frames, int num_hypotheses);
int vgg_p3p_ransac(const double* points2D_normalized, const double* points3D, const uint8_t* candidate_mask,
                   const int32_t* samples, int num_frames, int frames_per_sample_set, int num_points, int num_hypotheses,
                   const double* max_error_sq, double* out_pose, int32_t* out_num_inliers, double* out_residual_sum,
                   int32_t* out_best, uint8_t* out_inlier_mask, void* workspace, void* stream);

/* Two-view stage in front of the path: estimate_fundamental = 7-point RANSAC + 8-point local
 * optimisation for all (query frame, other frame) pairs at once   vggsfm/two_view_geo/fundamental.py:43-183,
 * two_view_geo/utils.py:63-298; caller estimate_preliminary.py:103-152 (-> fmat_inlier_mask).  PARITY PARTLY PINNED
 * (oracle/fundamental.py: Sampson distance, 8-point fit and winner selection checked against the reference's own functions;
 * the 7-point solver and the RNG are not -- kornia is absent); float64 here.
 * points1 / points2 [num_pairs][num_points][2] f64 pixels; valid_mask [num_pairs][num_points] uint8 or NULL
 * (matches with vis >= 0.05 and score >= 0.5, estimate_preliminary.py:118-126); matrices are 9 doubles row-major,
 * unit Frobenius norm, x2^T F x1 = 0.
 *  vgg_fmat_seven_point  samples [num_samples][7] int32 shared by all pairs (fundamental.py:67-75) ->
 *                        out_fmat [num_pairs][num_samples][3][9], out_valid [..][3] (1..3 real roots of the cubic)
 *  vgg_fmat_score        squared Sampson distance (utils.py:90-172) of every match under every hypothesis; inliers
 *                        <= max_error_sq and valid; out_counts [num_pairs][num_hypotheses] (-1 for an invalid
 *                        hypothesis), out_residual_sums = sum of the inlier residuals (-> the mean that breaks ties,
 *                        utils.py:63-87)
 *  vgg_fmat_eight_point  for each selected [num_pairs][num_selected] index into src_fmat [num_pairs][num_src][9]: the
 *                        8-point fit (masked normalisation, smallest eigenvector of X^T X, rank 2; fundamental.py:261-334)
 *                        on the inliers of that hypothesis, recomputed on the fly; selected entries whose src_counts is
 *                        negative give an invalid result
 *  vgg_fmat_residuals    fmat [num_pairs][9] -> out_residuals [num_pairs][num_points] (1e6 for invalid matches)
 * The caller sorts the counts (stable, descending) to select the lo_num best hypotheses between the calls. */
int vgg_fmat_seven_point(const double* points1, const double* points2, const int32_t* samples, int num_pairs, int num_points,
                         int num_samples, double* out_fmat, uint8_t* out_valid, void* stream);
int vgg_fmat_score(const double* points1, const double* points2, const uint8_t* valid_mask, const double* fmat,
                   const uint8_t* fmat_valid, int num_pairs, int num_points, int num_hypotheses, double max_error_sq,
                   int32_t* out_counts, double* out_residual_sums, void* stream);
int vgg_fmat_eight_point(const double* points1, const double* points2, const uint8_t* valid_mask, const double* src_fmat,
                         const int32_t* src_counts, const int32_t* selected, int num_pairs, int num_points, int num_src,
                         int num_selected, double max_error_sq, double* out_fmat, uint8_t* out_valid, void* stream);
int vgg_fmat_residuals(const double* points1, const double* points2, const uint8_t* valid_mask, const double* fmat, int num_pairs,
                       int num_points, double* out_residuals, void* stream);

/* Optional per-kernel timing (HIP events recorded on the launch stream around the dominant kernels).
 * kernel_id: 0 cam_pass<linearize> 1 point_pass 2 cam_pass<rhs> 3 schur_tile<off-diagonal tiles> 4 cholesky (all
 * launches of one solve) 5 point_step 6 schur_tile<diagonal tiles>.  vgg_ba_profile_read synchronises on the
 * recorded events. */
/* Launch choices the solver otherwise makes from the problem's shape (process-wide; for tests and measurements):
 * lanes_per_point 8 | 16 | 32 | 64 (0 = from the mean track length) -- lanes of a wavefront that share one point in the point
 * passes; long_tracks 1 / 0 (-1 = automatic) -- the variants that prefetch four observations per lane and keep no cached
 * Jacobians; cam_workgroups / point_workgroups (0 = automatic) -- total workgroups of the camera / point passes.  Every
 * combination computes the same iteration up to the order of its sums. */
int vgg_ba_tuning(int lanes_per_point, int long_tracks, int cam_workgroups, int point_workgroups);
/* Where F^T (r - E h) (and, with a shared camera, the intrinsics border of the reduced system) come from: 2 (default)
 * = from the diagonal Schur tile launch for every block shape -- 6 x 6 blocks
 * (shared or constant intrinsics, compressed factors): two wavefronts of a diagonal-tile workgroup multiply the staged segments
 * by a 3 x 3 per-point block on the side, + per-point sums of the point pass; 7 x 7 / 8 x 8 blocks (per-camera intrinsics, full
 * factors; round 6): every thread adds one tile row's products for two of a batch's entries -- no second camera-major evaluation
 * of the projections per iteration; 1 = the tile launch for 6 x 6 blocks only, the camera pass cam_pass<RHS> for the others (the
 * round-4/5 behaviour); 0 = the camera pass always.  All compute the same system up to the order of its sums.  Requires
 * entries[e][0] = the entry's point.
 * Bit 2 (value | 4; A/B measurements and tests): keep the glue of an LM iteration as separate launches -- tile sums, assembly,
 * preparation, step sums -- instead of the merged ones; the same bits either way.
 * Host-side state (the only one of this API): vgg_ba_begin notes, per WORKSPACE ADDRESS, that the preparation launch is still
 * due in front of the first point pass, and whether every camera group has a diagonal tile -- for which it copies the tile
 * table (16 bytes per tile) to the host and synchronises the stream ONCE per solve.  The table holds the 64 most recently begun
 * workspaces (mutex-protected, oldest replaced first); an entry lives until vgg_ba_begin is called again on that address or 64
 * other workspaces have begun.  A phase call on a workspace the table does not know takes the separate launches: same results,
 * three launches more per iteration. */
int vgg_ba_set_tile_rhs(int enable);
int vgg_ba_profile(int enable, int max_launches_per_kernel);
int vgg_ba_profile_read(int kernel_id, double* total_ms, int* launches, int reset);

/* Dense symmetric positive-definite solve of the reduced camera system (exposed for tests):
 * A (n,n) row-major lower triangle is overwritten by its Cholesky factor, b by the solution
 * (if b == A + n*n the forward substitution is fused into the factorisation).
 * workspace: vgg_cholesky_workspace_bytes(n) device bytes (inverse diagonal blocks).
 * *device_fail (int32, device) is set non-zero on a non-positive pivot (2: a hand-off of the single-launch form timed out).
 * n >= 128 with b behind A runs as ONE launch (a workgroup per 64 x 64 tile, hand-offs through per-tile flags); the sums of
 * a tile are taken in a fixed order that depends on the structure passed (split / envelope) only: the factor is reproducible
 * run to run, and equal to the plain entry's up to the rounding of those sums. */
size_t vgg_cholesky_workspace_bytes(int n);
int vgg_cholesky_solve(double* A, double* b, int n, void* workspace, int32_t* device_fail, void* stream);
/* the same with a block-diagonal leading part: A[i][j] = 0 for split_a <= i < split_a + split_b, j < split_a (exposed
 * for tests; see vgg_ba_problem.chol_split_a).  The split is a scheduling hint of the single-launch form (b == A + n * n);
 * with a separate b the system is factored in plain order. */
int vgg_cholesky_solve_split(double* A, double* b, int n, int split_a, int split_b, void* workspace, int32_t* device_fail,
                             void* stream);
/* the same with a row envelope: first_blk[r] (device, ceil(n / 64) entries) = first 64-column block in which rows
 * 64 r .. 64 r + 63 of A can be non-zero (see vgg_ba_problem.chol_first_blk); b must be stored directly behind A
 * (b == A + n * n) and n >= 128 for the envelope to be used (exposed for tests).  With an envelope the tiles are launched
 * in the order of their dependency depth and those outside it are not launched at all (one small set-up launch per call) */
int vgg_cholesky_solve_envelope(double* A, double* b, int n, const int32_t* first_blk, void* workspace, int32_t* device_fail,
                                void* stream);

/* ------------------------------------------------------------------------------------------
 * Dense depth alignment (the reference's dense_depth stage)
 *   extract_sparse_depth_and_point_from_reconstruction   vggsfm/runners/runner.py:744-772
 *   align_dense_depth_maps                                vggsfm/utils/utils.py:635-770
 * All pointers are device memory.  Images are indexed 0 .. num_images-1 by the caller; ragged disparity maps live in
 * one flat float32 buffer, image i at disp_off[i] with heights[i] x widths[i] pixels, row-major.
 *
 * Sparse depths: one row per observation, rows grouped by image by the caller (obs_image ascending; within an image the
 * reference's point-major order).  xyz (P,3) point rows, obs_point / obs_image (O) int32, point_id (O) int64, pose (S,3,4)
 * [R|t], cam (S,4) f, cx, cy, k (k = 0 for SIMPLE_PINHOLE).  Out: uvd (O,3) distorted pixel + depth, xyzid (O,4). */
int vgg_sparse_depth(const double* xyz, const int32_t* obs_point, const int32_t* obs_image, const int64_t* point_id,
                     const double* pose, const double* cam, long num_obs, double* uvd, double* xyzid, void* stream);
/* Per-image RANSAC fit disparity ~ scale * (1 / depth) ... as scikit-learn 1.7's RANSACRegressor(LinearRegression(),
 * min_samples=2, residual_threshold=median(1/depth)/30, max_trials, loss="squared_error"), one workgroup per image, all
 * images in one launch.  uvd (O,3) grouped by image: image i owns rows obs_ptr[i] .. obs_ptr[i+1] (obs_ptr int64,
 * num_images + 1).  draws (num_images, num_draws, 2) int32 indices into the image's kept rows (scikit-learn's recorded
 * sample_without_replacement draws), or NULL: draws from a counter-based generator keyed by `seed`.
 * Out per image: scale, shift (float32), n_trials, n_inliers, n_kept, status (0 ok, 1 no observation, 2 ill-posed
 * (non-finite data or threshold <= 0), 3 no consensus set, 4 fewer than 2 kept rows, 5 draws exhausted, 6 draw out of
 * range); per observation: kept (passed the bounds / positive-disparity filter), inlier (in the final consensus set).
 * workspace: vgg_depth_align_workspace_bytes(num_obs) device bytes. */
size_t vgg_depth_align_workspace_bytes(long num_obs);
int vgg_depth_align(const float* disp, const int64_t* disp_off, const int32_t* heights, const int32_t* widths,
                    const double* uvd, const int64_t* obs_ptr, int num_images, long num_obs, const int32_t* draws,
                    int num_draws, unsigned long long seed, int max_trials, float* scale, float* shift, int32_t* n_trials,
                    int32_t* n_inliers, int32_t* n_kept, int32_t* status, uint8_t* kept, uint8_t* inlier, void* workspace,
                    size_t workspace_bytes, void* stream);
/* In place on disp (numpy float32 semantics): nonzero d -> d * scale[i] + shift[i]; outside (0, 1e4] -> 0; depth (same
 * layout, float32) = 1 / d where d != 0 (an infinite quotient -> 0), else 0.  max_pixels = max_i heights[i] * widths[i]. */
int vgg_depth_apply(float* disp, float* depth, const int64_t* disp_off, const int32_t* heights, const int32_t* widths,
                    int num_images, long max_pixels, const float* scale, const float* shift, void* stream);
/* Back-projection of num_pixels valid pixels: pixels (N) int64 row-major index inside image pixel_image (N) int32;
 * normalised point by COLMAP's iterative undistortion (per point), times depth, then inv_pose (S,3,4) = [R^T | -R^T t].
 * Out xyz (N,3) float64. */
int vgg_depth_unproject(const int64_t* pixels, const int32_t* pixel_image, long num_pixels, const float* depth,
                        const int64_t* disp_off, const int32_t* widths, const double* cam, const double* inv_pose,
                        double* xyz, void* stream);

/* ------------------------------------------------------------------------------------------
 * Reprojection video (the reference's make_reproj_video stage)
 *   create_video_with_reprojections   vggsfm/utils/utils.py:428-546
 *   filter_invisible_reprojections    vggsfm/utils/utils.py:393-425
 * All pointers are device memory.  color_mode: 0 dis_to_center, 1 dis_to_origin, 2 point_order.
 *
 * Colour statistics over all num_points (> 0) points of the model, float64 as numpy computes them, into
 * stats[VGG_REPROJ_STATS]: [0..2] np.median(xyz, axis=0) (mode 0; else 0), [3] min_dis, [4] max_dis (mode 0: min and
 * np.percentile(., 95) of the distances to the median; mode 1: min and max of the norms; mode 2: 0), [5] the largest point
 * id (mode 2; else 0).  xyz (P,3) (modes 0, 1), point_id (P) int64 (mode 2).  Four launches, no host round trip.
 * workspace: vgg_reproj_stats_workspace_bytes(num_points) device bytes. */
#define VGG_REPROJ_STATS 8
#define VGG_REPROJ_MAX_RADIUS 32
size_t vgg_reproj_stats_workspace_bytes(long num_points);
int vgg_reproj_stats(const double* xyz, const int64_t* point_id, long num_points, int color_mode, double* stats,
                     void* workspace, size_t workspace_bytes, void* stream);
/* Centres, colours and per-pixel visibility of the observations of frames frame_begin .. frame_end-1.  Frame f owns the
 * observation rows obs_range[2f] .. obs_range[2f+1] of uvd (O,3) [u, v, depth] and xyzid (O,4) [x, y, z, point id]
 * (O < 2^31); its grid window, (heights[f] + 2r) x (widths[f] + 2r) cells with cell (gx, gy) = integer centre (gx - r,
 * gy - r), starts at grid_off[f] - grid_off[frame_begin] (grid_off int64, prefix of the window sizes); chunk_cells =
 * grid_off[frame_end] - grid_off[frame_begin] (< 2^31), max_frame_obs = the largest observation count of the chunk.
 * Centre: rint(u), rint(v) (half to even).  An observation whose centre lies outside its window cannot touch its image and
 * gets obs_cell = -1; in the window, the cell's winner is the smallest depth, ties to the lowest row, -0.0 == +0.0, a NaN
 * depth first (np.argmin).  grid_key (uint64) / grid_obs (uint32) hold chunk_cells cells each and are overwritten (the
 * winner's row, 0xffffffff where none).  Colour (when lut != NULL): matplotlib's Colormap.__call__ of the colour index
 * (stats from vgg_reproj_stats), looked up in lut (lut_n + 3 entries: the colormap's N colours, under, over, bad; each
 * int(255 * channel) as r | g << 8 | b << 16) into color (O).  Optional: centers (O,2) int32 (INT32_MIN outside the window),
 * visible (O) uint8 (1 = drawn).  draw_radius <= VGG_REPROJ_MAX_RADIUS. */
int vgg_reproj_visible(const double* uvd, const double* xyzid, const int64_t* obs_range, const int32_t* heights,
                       const int32_t* widths, const int64_t* grid_off, int frame_begin, int frame_end, long max_frame_obs,
                       long chunk_cells, int draw_radius, int color_mode, const double* stats, const uint32_t* lut,
                       int lut_n, int32_t* obs_cell, uint32_t* color, int32_t* centers, uint8_t* visible,
                       unsigned long long* grid_key, uint32_t* grid_obs, void* stream);
/* Padded BGR canvases (frame_end - frame_begin, canvas_h, canvas_w, 3) uint8 into out, after vgg_reproj_visible on the same
 * frames and grid: zero outside the centred image (top = (canvas_h - h) / 2, left = (canvas_w - w) / 2), inside it the
 * RGB source pixel (images: flat uint8, frame f at img_off[f], heights[f] x widths[f] x 3) flipped to BGR, with every
 * winning circle within draw_radius composited in row order: coverage k = the number of i, j in 0..3 with
 * (8(x - cx) + 2i - 3)^2 + (8(y - cy) + 2j - 3)^2 <= 64 r^2 (r = 0: k = 16 at the centre), out = (old (16 - k) + c k + 8) >> 4
 * per channel, colour channel 0 into canvas channel 0. */
int vgg_reproj_draw(const uint8_t* images, const int64_t* img_off, const int32_t* heights, const int32_t* widths,
                    const int64_t* grid_off, int frame_begin, int frame_end, int canvas_h, int canvas_w, int draw_radius,
                    const uint32_t* grid_obs, const uint32_t* color, uint8_t* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Point colours of the video path
 *   VideoRunner._update_points_color   vggsfm/runners/video_runner.py:475-492
 * All pointers are device memory.  The observation table is point-major: obs_point (O) int64 ascending (ties in
 * ascending frame), obs_frame (O) int64, obs_uv (O,2) float32; O < 2^31, points 0 .. num_points-1.
 *
 * Gather, frame-major: rows row_begin .. row_end-1 of order (a permutation of 0 .. O-1 grouping the observations by
 * frame) must be observations of frames frame_begin .. frame_end-1, and frames holds exactly those frames as
 * (frame_end - frame_begin, 3, height, width) float32.  For each such observation o: u = floor(uv[0]), v = floor(uv[1])
 * as int64; if v < height and u < width (no lower bound) it contributes images[f, :, v, u] (reverse: [f, :, u, v]), a
 * negative index counting from the end as in Python.  gathered (O,4) float32 row o = (r, g, b, 1) when it contributes,
 * else (0, 0, 0, 0).  An index still out of range after wrapping (the reference's IndexError), or a row whose frame lies
 * outside the chunk: atomicMin(bad_obs, o), the row is written as not contributing.  The caller sets *bad_obs = INT32_MAX
 * before the first chunk.  Every chunk writes only its own rows, so any split of the frames gives the same buffer. */
int vgg_color_gather(const float* frames, int frame_begin, int frame_end, int height, int width, int reverse,
                     const int64_t* order, long row_begin, long row_end, const int64_t* obs_frame, const float* obs_uv,
                     long num_obs, float* gathered, int32_t* bad_obs, void* stream);
/* Per point, after the gathers of every frame: rgb (P,3) float32 = the float32 sum of the contributing rows of gathered,
 * in table order, divided by their count; (0, 0, 0) and has_color = 0 for a point without one (has_color (P) uint8,
 * else 1).  point_ptr: workspace of num_points + 1 int64 (overwritten with the point-major row offsets).  Two launches. */
int vgg_color_reduce(const int64_t* obs_point, long num_obs, long num_points, const float* gathered, int64_t* point_ptr,
                     float* rgb, uint8_t* has_color, void* stream);

/* ------------------------------------------------------------------------------------------
 * Track video
 *   Visualizer.draw_tracks_on_video   vggsfm/utils/visualizer.py:163-295, as runner.py:445-450 calls it
 * All pointers are device memory.  T frames of height x width; the canvas is (height + 2 pad) x (width + 2 pad).
 * Every track's prediction is drawn per frame as PIL's ellipse of integer radius r around its integer centre, in track
 * order, opaque: a pixel ends with the colour of the highest track index whose stencil covers it.
 *
 * Owner pass over frames frame_begin .. frame_end-1 (at most 65535) of tracks (T, num_tracks, 2), float32 or float64
 * (tracks_f64): centre = (int64)(coordinate + pad), the addition in the tracks' precision, truncated toward zero.  A
 * track of a frame below query_frame, one whose integer x or y is 0, or whose coordinate is not finite or beyond 2^62
 * draws nothing.  visibility (T, num_tracks) of vis_kind, or NULL with VGG_TRACK_VIS_NONE: a zero (-0.0 too) selects
 * the outline stencil, anything else (a NaN included) the filled one.  stencil_rows: 2 x (2r + 1) uint32 in host
 * memory, the filled stencil's rows then the outline's, row dy + r, bit dx + r.  owner (frame_end - frame_begin,
 * canvas_h, canvas_w) uint32 (< 2^31 cells) is cleared by the entry and ends as track index + 1 of each pixel's
 * winner, 0 where nothing was drawn.  num_tracks < 2^31 - 1, radius <= VGG_TRACK_MAX_RADIUS. */
#define VGG_TRACK_MAX_RADIUS 15
#define VGG_TRACK_VIS_NONE 0
#define VGG_TRACK_VIS_U8 1
#define VGG_TRACK_VIS_F32 2
#define VGG_TRACK_VIS_F64 3
int vgg_track_owner(const void* tracks, int tracks_f64, const void* visibility, int vis_kind, int frame_begin, int frame_end,
                    int query_frame, long num_tracks, int pad, int canvas_h, int canvas_w, int radius,
                    const uint32_t* stencil_rows, uint32_t* owner, void* stream);
/* Resolve pass, after vgg_track_owner on the same frames: frames holds frames frame_begin .. frame_end-1 as
 * (n, 3, height, width) float32 or uint8 (frames_u8).  Output pixel = the colour of its owner (colors[owner - 1], or
 * colors[frame] with color_per_frame; r | g << 8 | b << 16), else the frame's pixel as uint8 (float: truncated, clamped
 * to 0..255, NaN -> 0), else 255 in the border of pad.  out is the whole video (T - 1 + first_copies, 3, canvas_h,
 * canvas_w) uint8: frame 0 is written first_copies (>= 1) times at its head, frame t > 0 at t - 1 + first_copies. */
int vgg_track_resolve(const void* frames, int frames_u8, int frame_begin, int frame_end, int height, int width, int pad,
                      const uint32_t* owner, const uint32_t* colors, int color_per_frame, int first_copies, uint8_t* out,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VGGSFM_AMD_H */
