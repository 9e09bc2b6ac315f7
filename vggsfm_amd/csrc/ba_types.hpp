// Bundle adjustment (ba*.hip): the constants, the workspace and launch types and the host helpers every BA unit shares,
// and the launchers through which the units talk to the driver (ba.hip).  A kernel is launched only from the unit that
// defines it; the kernel -> file map is in DESIGN.md.  Nothing here may be `static`: a static object or function in this
// header would give every unit a copy of its own (g_tuning, g_prof: ONE definition, in ba.hip).
#pragma once
#include <type_traits>

#include "camera_model.hpp"
#include "../../include/vggsfm_amd.h"

namespace vgg {

// chol.hip
int cholesky_solve_enqueue(double* A, double* b, int n, double* inv_blocks, int32_t* device_fail, const int32_t* skip_flag,
                           hipStream_t st, const CholOverlap* overlap, int split_a, int split_b, const int32_t* first_blk,
                           bool flags_cleared);
int32_t* cholesky_dataflow_flags(double* ws, int n, size_t* count);
size_t cholesky_workspace_bytes(int n);
void dataflow_signal(int32_t* flag, hipStream_t st);

constexpr int kGroup = 16;       // cameras per Schur tile side
constexpr int kSub = 32;         // entries per strided sub-chunk of a Schur workgroup (see schur_tile_kernel)
constexpr int kMaxWG = 2048;
constexpr int kCamSplitMax = 16;  // workgroups per camera in the camera passes
constexpr int kCamNV = 48;        // >= values a camera pass accumulates (BD(BD+1)/2 + BD + 1 <= 45)
constexpr int kPackPad = 1024;    // >= ranks of a sharded solve (padding of the packed reduced system to equal slices)

struct Ctl {
  double radius, decrease_factor, x_cost, initial_cost, gmax_cams, gmax, cand_cost, mcc, step_norm, rel;
  int32_t iteration, done, termination, need_lin, scale_ready, invalid_streak, num_succ, num_unsucc;
  int32_t linear_fail, accept, rank, world, grad_logged;
  int32_t step_arrivals;          // cam_reduce workgroups of the candidate's linearisation that have stored (the last one sums)
  // how often this solve ran the merged glue: tile_assemble_kernel launches, step sums in cam_reduce_kernel (tests read them)
  int32_t merged_glue_launches, merged_step_sums;
  int32_t fused_step_prologues;   // point_step launches of this solve that ran cam_update's body in their prologue (tests read it)
};

struct Dims {
  int C, P, O, NI, model, kd, only_k, shared, BDp, n_red, kdsh, loss;
  double loss_scale;
};

// Doubles per slot (one observation) of the segment buffer Y.
// 6 x 6 camera blocks (shared or constant intrinsics): COMPRESSED -- the 6 x 3 Schur factor of an observation is
//   Y_i = s_c o (F_i^T E_i G_p) = s_c o [ [2 a]x ; I ] N_i,   N_i = Jw^T (E_i G_p) (3 x 3),  a = R_c X_p,
// because the pose Jacobian factors as F = Jw [ -2 [a]x | I ] (J_delta = -2 J_Y [R X]x, J_t = J_Y; the
// loss corrector multiplies from the left).  The slot holds N (row-major, 9) and 2 a (3): 96 bytes instead of 144; the tile
// kernel rebuilds the six rows while it stages the segment, the Jacobi scales s_c and the constant-parameter masks are
// applied to the finished tile sums (tile_reduce_kernel).  Larger blocks (per-camera intrinsics) keep the full factor.
constexpr int kYc = 12;
inline size_t y_slot_doubles(const Dims& d) { return (d.shared || d.kd == 0) ? (size_t)kYc : (size_t)d.BDp * 3; }

struct Ws {  // device workspace carve-up (pointers into the caller's buffer)
  Ctl* ctl;
  vgg_ba_iteration* log;
  double *cand_q, *cand_t, *cand_intr, *cand_pts;
  double *scale_c, *scale_p, *colsq_c, *dsq_c, *dy;
  uint8_t* active;            // [n_red]
  double* lin;                // reduce buffer 0: U[C][BDp*BDp] | g[C][BDp] | cost[C]
  double *U, *g, *costc;
  double* sys;                // reduce buffer 1: S[n*n] | rhs[n]
  double *S, *rhs;
  double* S2;                 // [n*n] sums of the tile batches that are computed while the factorisation runs (overlap mode)
  double* gmax_pts;           // reduce buffer 2 (MAX): 1 double (padded to 8)
  double* stepsum;            // reduce buffer 3: cost, mcc, step_sq, xnorm_sq  (padded to 8)
  double *G, *hs, *Ms;        // per point: 6, 3, 3*kdsh
  double *pdamp;              // per point: the damping of its block in unscaled coordinates, D^2 = dd / s^2 (3)
  double* T;                  // [C][BDp][1+kdsh]
  double* part_B;             // [kMaxWG] per-workgroup gradient max
  double* part_F;             // [kMaxWG][4]
  double* packed;             // lower triangle of S (row by row) + rhs: the multi-GPU reduce payload, followed by 2 kPackPad
  size_t packed_count;        //   doubles of padding (the reduce-scatter input is W equal slices: W ceil(count / W) doubles)
  double* pk_mine;            // [ceil(count / W) + 1] this rank's reduced slice + its local gradient maximum (reduce-scatter
                              //   output = all-gather input)
  double* pk_gathered;        // [W (ceil(count / W) + 1)] the all-gather output, read in place by the unpack (phase 6)
  double* cam_part;           // [C+1][3] step^2 / x^2 of camera-side parameters, camera-side share of the model cost change
  double* cam_split;          // [C][kCamSplitMax][kCamNV] partial sums of the split camera passes
  double* Y;                  // [num_segments][16][BDt*3] zero-padded per-observation Schur factors s_c o (F^T E G_p)
  size_t y_bytes;
  double* chol_inv;           // inverse diagonal blocks of the Cholesky factor
  double* tile_part;          // [num_chunks][R][R] partial Schur tiles, R = 16*BDt
  int32_t* batch_flags;       // [8] overlap mode: tile batch b >= 1 has been summed into S2 (raised by a kernel behind it)
  // reduced right-hand side from the diagonal tiles (tile_rhs, see schur_tile_body): per point Z = [z | y_0 | y_1] (3 x 3,
  // column-major) with E hs = E G z, E Ms_m = E G y_m; per diagonal chunk the sums over its entries of Y_seg Z (96 x 3);
  // per point-pass workgroup the shared-intrinsics terms sum_p Wa_p hs_p (KD) and sum_p Wa_p Ms_p^T (KD x KD)
  double *Zp, *rz_part, *part_Q;
  unsigned long long* split_off;   // split exchange: [2][n + 2] elements of part A / B in the rows above row i (i = n: the rhs; i = n + 1: the part's total)
  double* rz;                 // [ceil(C / 16)][96 x 3] rz_part summed over the chunks of a group's diagonal tile (tile_reduce_kernel)
  int tile_rhs;               // 1: cam_pass<RHS> is not launched, its sums come from the diagonal tile launch + point_pass
  // the linearisation at the candidate (cam_pass<CAND>, same layout as `lin`): carved behind everything else so that no
  // other buffer moves; commit_kernel copies it into `lin` when the step is accepted
  double* lin_cand;
  double *U_cand, *g_cand, *cost_cand;
  size_t lin_count, sys_count, total_bytes;
};

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }


inline Dims make_dims(const vgg_ba_problem* pb) {
  Dims d;
  d.C = pb->num_cams; d.P = pb->num_pts; d.O = pb->num_obs; d.NI = pb->num_intr; d.model = pb->camera_model;
  const int rf = pb->refine_focal ? 1 : 0, rk = (pb->refine_extra && pb->camera_model == kSimpleRadial) ? 1 : 0;
  d.kd = rf + rk;
  d.only_k = (!rf && rk) ? 1 : 0;
  d.shared = (pb->num_intr == 1) ? 1 : 0;
  d.BDp = 6 + d.kd;
  d.n_red = 6 * d.C + d.kd * d.NI;
  d.kdsh = d.shared ? d.kd : 0;
  d.loss = pb->loss; d.loss_scale = pb->loss_scale;
  return d;
}

// overrides of the automatic launch choices (vgg_ba_tuning, vgg_ba_set_tile_rhs): 0 / -1 = automatic
// legacy_glue (vgg_ba_set_tile_rhs(| 4), A/B runs and tests): tile sums, assembly, preparation and the step sums as the separate
// launches they were before they were merged (tile_assemble_kernel, cam_reduce_kernel's last arriver)
struct Tuning { int lpp, longt, cam_wgs, point_wgs, tile_rhs, legacy_glue; };
extern Tuning g_tuning;   // (defined in ba.hip)

inline Ws carve(const Dims& d, int max_iters, int num_chunks, int num_segments, void* base) {
  Ws w;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return (char*)base + o; };
  w.ctl = (Ctl*)take(sizeof(Ctl));
  w.log = (vgg_ba_iteration*)take(sizeof(vgg_ba_iteration) * (size_t)(max_iters + 2));
  w.cand_q = (double*)take(8ull * 4 * d.C); w.cand_t = (double*)take(8ull * 3 * d.C);
  w.cand_intr = (double*)take(8ull * 4 * d.NI); w.cand_pts = (double*)take(8ull * 3 * d.P);
  w.scale_c = (double*)take(8ull * d.n_red); w.scale_p = (double*)take(8ull * 3 * d.P);
  w.colsq_c = (double*)take(8ull * d.n_red); w.dsq_c = (double*)take(8ull * d.n_red);
  w.dy = (double*)take(8ull * d.n_red);
  w.active = (uint8_t*)take(d.n_red);
  w.lin_count = (size_t)d.C * d.BDp * d.BDp + (size_t)d.C * d.BDp + d.C;
  w.lin = (double*)take(8ull * w.lin_count);
  w.U = w.lin; w.g = w.U + (size_t)d.C * d.BDp * d.BDp; w.costc = w.g + (size_t)d.C * d.BDp;
  w.sys_count = (size_t)d.n_red * d.n_red + d.n_red;
  w.sys = (double*)take(8ull * w.sys_count);
  w.S = w.sys; w.rhs = w.S + (size_t)d.n_red * d.n_red;
  w.S2 = (double*)take(8ull * (size_t)d.n_red * d.n_red);
  w.packed_count = (size_t)d.n_red * (d.n_red + 1) / 2 + d.n_red;
  // padding for W <= kPackPad ranks: the one-piece exchange needs W c <= count + W - 1 in `packed` and W (c + 1) <= count + 2W - 1
  // in `pk_gathered`; the split exchange rounds two parts up, W (ca + cb) <= count + 2 (W - 1) and W ca + W (cb + 1) <= count + 3W - 2
  w.packed = (double*)take(8ull * (w.packed_count + 2 * kPackPad));
  w.pk_mine = (double*)take(8ull * (w.packed_count + 2));                      // (W = 1: the whole payload)
  w.pk_gathered = (double*)take(8ull * (w.packed_count + 3 * kPackPad));
  w.gmax_pts = (double*)take(64);
  w.stepsum = (double*)take(64);
  w.G = (double*)take(8ull * 6 * d.P); w.hs = (double*)take(8ull * 3 * d.P);
  w.pdamp = (double*)take(8ull * 3 * d.P);
  w.Ms = (double*)take(8ull * 3 * (d.kdsh ? d.kdsh : 1) * d.P);
  w.T = (double*)take(8ull * d.C * d.BDp * (1 + d.kdsh));
  w.part_B = (double*)take(8ull * kMaxWG);
  w.part_F = (double*)take(8ull * kMaxWG * 4);
  w.cam_part = (double*)take(8ull * (d.C + 1) * 3);
  w.cam_split = (double*)take(8ull * (size_t)d.C * kCamSplitMax * kCamNV);
  // + one all-zero segment behind the last real one (target of the tile kernel's loads past the end of a list)
  w.y_bytes = 8ull * ((size_t)(num_segments > 0 ? num_segments : 0) + 1) * kGroup * y_slot_doubles(d);
  w.Y = (double*)take(w.y_bytes);
  w.chol_inv = (double*)take(cholesky_workspace_bytes(d.n_red));
  {
    const size_t bdt = d.shared ? 6 : d.BDp;
    w.tile_part = (double*)take(8ull * (size_t)(num_chunks > 0 ? num_chunks : 1) * bdt * bdt * 256);   // R*R, R = 16*bdt
  }
  w.batch_flags = (int32_t*)take(64);
  w.Zp = (double*)take(8ull * 9 * (d.P > 0 ? d.P : 1));
  w.rz_part = (double*)take(8ull * (size_t)(num_chunks > 0 ? num_chunks : 1) * kGroup * 6 * 3);
  w.part_Q = (double*)take(8ull * kMaxWG * 8);
  w.rz = (double*)take(8ull * (size_t)((d.C + kGroup - 1) / kGroup) * kGroup * 6 * 3);
  w.split_off = (unsigned long long*)take(8ull * 2 * ((size_t)d.n_red + 2));
  w.lin_cand = (double*)take(8ull * w.lin_count);
  w.U_cand = w.lin_cand; w.g_cand = w.U_cand + (size_t)d.C * d.BDp * d.BDp; w.cost_cand = w.g_cand + (size_t)d.C * d.BDp;
  w.tile_rhs = 0;
  w.total_bytes = off;
  return w;
}

struct DevProblem {  // by-value kernel argument
  Dims d;
  const double *cam_q, *cam_t, *intr, *pts;
  const int32_t *row_ptr, *obs_cam, *col_ptr, *cobs_pt, *obs_slot;
  const float2 *obs_uv, *cobs_uv;
  const uint8_t *cam_const, *intr_const, *pt_const;
};

inline DevProblem dev_problem(const vgg_ba_problem* pb, const Dims& d) {
  DevProblem p;
  p.d = d; p.cam_q = pb->cam_q; p.cam_t = pb->cam_t; p.intr = pb->intr; p.pts = pb->pts;
  p.row_ptr = pb->row_ptr; p.obs_cam = pb->obs_cam; p.col_ptr = pb->col_ptr; p.cobs_pt = pb->cobs_pt;
  p.obs_slot = pb->obs_slot;
  p.obs_uv = (const float2*)pb->obs_uv; p.cobs_uv = (const float2*)pb->cobs_uv;
  p.cam_const = pb->cam_const; p.intr_const = pb->intr_const; p.pt_const = pb->pt_const;
  return p;
}

// Lanes per point of the point passes from the mean track length (vgg_ba_tuning overrides).  A point's lanes share
// its serial work (reductions, 3 x 3 factorisation), which outweighs the sweeps over its observations up to ~70 of them:
// measured per LM iteration, point_pass + point_step -- c2 (mean 12.5 observations) 64: 0.112, 32: 0.075, 16: 0.065,
// 8: 0.059 ms; c3 (mean 50) 64: 0.674, 32: 0.549, 16: 0.499, 8: 0.535 ms; one c4 shard (mean 100) 32: 0.509, 16: 0.544 ms.
inline int lanes_per_point(int P, int O) {
  const int forced = g_tuning.lpp;
  if (forced == 8 || forced == 16 || forced == 32 || forced == 64) return forced;
  const double mean = P > 0 ? (double)O / P : 64.0;
  return mean <= 72.0 ? 16 : 32;
}
// long-track variants of the point passes (four prefetched observations per lane, no cached Jacobians)
inline bool long_tracks(int lpp, int P, int O) {
  return g_tuning.longt >= 0 ? g_tuning.longt != 0 : (double)O > 1.5 * lpp * (double)P;
}

// workgroups per camera of the camera passes: ~1024 workgroups in total for a large problem (c3: 19 observations per
// thread; 2048 workgroups cost 0.117 + 0.131 ms, 1024: 0.099 + 0.128, 512: 0.105 + 0.146), at least ~2048 observations per
// workgroup for a small one (c2: 512 workgroups 0.025 + 0.019 ms, 1024: 0.038 + 0.026).  vgg_ba_tuning overrides the total.
inline int cam_split_for(int C, int O) {
  const int target = g_tuning.cam_wgs > 0 ? g_tuning.cam_wgs : min(1024, max(256, O / 2048));
  const int s = target / (C > 0 ? C : 1);
  return s < 1 ? 1 : (s > kCamSplitMax ? kCamSplitMax : s);
}

// Optional per-kernel timing with HIP events recorded on the launch stream (bench.py's roofline leg).
enum { kProfLinearize = 0, kProfPointPass, kProfCamRhs, kProfSchurTile, kProfCholesky, kProfPointStep,
       kProfSchurTileDiag, kProfCount };   // kProfSchurTile = the off-diagonal launch
struct Profiler {
  bool on = false;
  int cap = 0;
  hipEvent_t* start[kProfCount] = {};
  hipEvent_t* stop[kProfCount] = {};
  int n[kProfCount] = {};
};
extern Profiler g_prof;   // (defined in ba.hip)
struct ProfScope {
  int id; hipStream_t st; bool live;
  ProfScope(int id_, hipStream_t st_) : id(id_), st(st_), live(g_prof.on && g_prof.n[id_] < g_prof.cap) {
    if (live) (void)hipEventRecord(g_prof.start[id][g_prof.n[id]], st);
  }
  ~ProfScope() {
    if (live) { (void)hipEventRecord(g_prof.stop[id][g_prof.n[id]], st); g_prof.n[id]++; }
  }
};

struct Launch {
  Dims d; DevProblem dp; Ws w; vgg_ba_options opt; hipStream_t st; int wgB;
  int lpp;                                      // lanes per point of the point passes: 16, 32 or 64 (lanes_per_point)
  const int32_t* chunk_desc; const int32_t* entries; int num_chunks, num_segments;
  int merged_tile_launch;
  const int32_t* tile_desc; int num_tiles;
  const int32_t* batches; int num_batches;      // HOST table [num_batches][6], see vgg_ba_problem.tile_batches
  int chol_split_a, chol_split_b;               // block-diagonal leading part of the reduced system (0 = none)
  const int32_t* chol_first_blk;                // row envelope of the reduced system in 64-column blocks (device) or NULL
  double *cam_q, *cam_t, *intr, *pts;
};

// run-time value -> template argument: the refined intrinsics per block (kd), the lanes per point of the point passes (lpp)
template <typename Fn>
inline void dispatch_kd(int kd, Fn fn) {
  switch (kd) {
    case 0: fn(std::integral_constant<int, 0>{}); break;
    case 1: fn(std::integral_constant<int, 1>{}); break;
    default: fn(std::integral_constant<int, 2>{}); break;
  }
}
template <typename Fn>
inline void dispatch_lpp(int lpp, Fn fn) {
  switch (lpp) {
    case 8: fn(std::integral_constant<int, 8>{}); break;
    case 16: fn(std::integral_constant<int, 16>{}); break;
    case 32: fn(std::integral_constant<int, 32>{}); break;
    default: fn(std::integral_constant<int, 64>{}); break;
  }
}

// The launchers: each enqueues kernels of its own unit on L.st (the tile batches: on `st`) and picks the instantiation from
// the run-time L.d.kd / L.lpp / ... itself.
// ba_cam.hip
void launch_linearize(const Launch& L, const DevProblem& dp, const Ws& w, int step_parts = 0);   // cam_pass<LIN / CAND> + cam_reduce
void launch_cam_rhs(const Launch& L);                 // cam_pass<RHS> + cam_reduce (without tile_rhs)
// ba_point.hip
void launch_point_pass(const Launch& L);
void launch_point_step(const Launch& L);              // (cam_update in front where point_step's prologue does not run its body)
void launch_reduce_step(const Launch& L);
// ba_tiles.hip
void launch_prep(const Launch& L);                    // (prep_kernel shares prep_body with tile_assemble_kernel: same unit)
void launch_schur_batches(const Launch& L, int b0, int b1, hipStream_t st, double* dst, int32_t* done_flags = nullptr,
                          int which = 0, bool sums = true);
void launch_assemble(const Launch& L);
void launch_tile_assemble(const Launch& L);
// ba_exchange.hip
void launch_pack_lower(const Launch& L, int mode);
void launch_split_offsets(const Launch& L);
void launch_pack_split(const Launch& L, int part, int mode);
size_t split_count_a(const Dims& d);

}  // namespace vgg
