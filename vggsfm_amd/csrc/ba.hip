// Levenberg-Marquardt bundle adjustment with a block-sparse Schur complement, gfx950 (CDNA4).
//
// Replaces pycolmap.bundle_adjustment / pycolmap.pose_refinement as the reference uses them
// (vggsfm/utils/triangulation.py:213,387,590,1050,1142; vggsfm/runners/video_runner.py:508,831,1001):
// COLMAP's BundleAdjuster on Ceres' trust-region LM.  The Ceres control flow that decides the
// trajectory (Jacobi scaling frozen at iteration 0, D^2 = clamp(diag J^T J)/radius, step quality,
// radius update, invalid steps) is restated on the device so that the host never synchronises inside
// the loop.  SURVEY.md Appendix A is the working spec.
//
// Data layout (all resident in HBM for the whole solve, float64 unless noted):
//   cameras   cam_q[C,4] cam_t[C,3] intr[NI,4]        replicated on every GPU
//   points    pts[P,3]                                 sharded by point index across GPUs
//   observations, twice:  point-major CSR (row_ptr, obs_cam i32, obs_uv f32x2)
//                         camera-major CSR (col_ptr, cobs_pt i32, cobs_uv f32x2)
//   reduced camera system S[n,n] (lower, row-major), n = 6C + kd*NI
// Kernels per LM iteration (algorithmic bytes in DESIGN.md):
//   cam_pass<LIN>   camera-major: U_c = F^T F, g_c = F^T r, cost            (vgg_ba_begin only: at the start point)
//   point_pass      point-major, one wavefront per point: V_p = E^T E + D^2, its Cholesky inverse,
//                   h_p = V^-1 E^T r, shared-intrinsics coupling
//   cam_pass<RHS>   camera-major: F^T (r - E h_p) and the shared-intrinsics Schur terms
//   schur_tile      S -= sum_p Y_p Y_p^T on 16x16-camera tiles; thread (a,b) owns the 6x6 (7x7, 8x8)
//                   block of cameras (I*16+a, J*16+b) in registers, Y blocks staged through LDS
//   assemble        diagonal blocks, damping, constant columns
//   cholesky        chol.hip (matrix-core trailing update)
//   point_step      back-substitution, model cost change, candidate points
//   cam_pass<CAND>  the same camera-major pass at the candidate: its cost decides the step, and on acceptance its U_c, g_c
//                   are the next linearisation (no pass at the start of the next iteration)
//   control         Ceres' accept / reject logic, one workgroup
// This file is the driver: the solve's own small kernels (init, begin_iteration, control, commit), the sequence of launches
// of an LM iteration (phase_schur, phase_step, phase_update) and every extern "C" entry.  The launches live with their
// kernels -- ba_cam.hip, ba_point.hip, ba_tiles.hip, ba_exchange.hip -- behind the launchers declared in ba_types.hpp.
#include <mutex>
#include <vector>

#include "ba_types.hpp"

namespace vgg {

// the one copy of the host state that the units share (ba_types.hpp declares them)
Tuning g_tuning = {0, -1, 0, 0, 2, 0};
Profiler g_prof;

// ---------------------------------------------------------------------------------------------
__global__ void init_kernel(DevProblem pb, Ws w, vgg_ba_options opt, int rank, int world) {
  const Dims& d = pb.d;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j == 0) {
    Ctl c;
    memset(&c, 0, sizeof(c));
    c.radius = opt.initial_trust_region_radius; c.decrease_factor = 2.0; c.need_lin = 1; c.rank = rank; c.world = world;
    *w.ctl = c;
    w.gmax_pts[0] = 0; for (int i = 0; i < 4; ++i) w.stepsum[i] = 0;
  }
  if (j < d.n_red) {
    bool act;
    if (j < 6 * d.C) {
      const int c = j / 6, k = j - 6 * c;
      const unsigned f = pb.cam_const ? pb.cam_const[c] : 0u;
      act = (pb.col_ptr[c + 1] > pb.col_ptr[c]) || world > 1;
      if (f & 1u) act = false;
      if (k >= 3 && (f & (2u << (k - 3)))) act = false;
    } else {
      const int a = (j - 6 * d.C) / d.kd;
      act = !(pb.intr_const && pb.intr_const[a]);
      if (!d.shared && world == 1 && !(pb.col_ptr[a + 1] > pb.col_ptr[a])) act = false;
    }
    w.active[j] = act ? 1 : 0;
    w.scale_c[j] = 1.0;
  }
}

// start-of-iteration checks (Ceres FinalizeIterationAndCheckIfMinimizerCanContinue)
__device__ __forceinline__ void begin_iteration(const Ws& w, const vgg_ba_options& opt) {
  Ctl* c = w.ctl;
  if (c->need_lin) {
    c->gmax = fmax(c->gmax_cams, w.gmax_pts[0]);
    w.log[c->iteration].gradient_max_norm = c->gmax;
    if (c->iteration == 0) {
      vgg_ba_iteration z;
      z.iteration = 0; z.successful = 1; z.cost = c->x_cost; z.cost_change = 0; z.gradient_max_norm = c->gmax;
      z.step_norm = 0; z.relative_decrease = 0; z.radius = c->radius;
      w.log[0] = z;
    }
    if (c->gmax <= opt.gradient_tolerance) { c->done = 1; c->termination = 1; return; }
  }
  if (c->iteration >= opt.max_num_iterations) { c->done = 1; c->termination = 0; return; }
  if (c->radius <= opt.min_trust_region_radius) { c->done = 1; c->termination = 4; return; }
  c->scale_ready = 1;
  c->need_lin = 0;
  c->iteration += 1;
}


// one workgroup: thread 0 runs the checks; then the constant / unobserved columns of the reduced system get a unit
// diagonal and a zero right-hand side (their Jacobian columns are zero)
__global__ __launch_bounds__(256) void begin_iteration_kernel(Ws w, vgg_ba_options opt, int n, int32_t* chol_flags, int chol_flag_count) {
  if (w.ctl->done) return;
  // the hand-off flags of the factorisation that follows (chol.hip, cholesky_dataflow_flags): cleared here, not by a fill launch
  for (int j = threadIdx.x; j < chol_flag_count; j += 256) chol_flags[j] = 0;
  if (threadIdx.x == 0) begin_iteration(w, opt);
  for (int j = threadIdx.x; j < n; j += 256) {
    if (w.active[j]) continue;
    w.S[(size_t)j * n + j] = 1.0;
    w.rhs[j] = 0.0;
  }
}

// Ceres' trust-region decision (TrustRegionMinimizer::Minimize body + LevenbergMarquardtStrategy)
__global__ __launch_bounds__(64) void control_kernel(Ws w, vgg_ba_options opt, int C) {
  Ctl* c = w.ctl;
  if (c->done) { if (threadIdx.x == 0) c->accept = 0; return; }   // (no-op iterations behind the end must not commit again)
  double step_c = 0, xn_c = 0, mcc_c = 0;
#pragma unroll 4
  for (int i = threadIdx.x; i <= C; i += 64) { step_c += w.cam_part[3 * i]; xn_c += w.cam_part[3 * i + 1]; mcc_c += w.cam_part[3 * i + 2]; }
  step_c = wave_sum(step_c); xn_c = wave_sum(xn_c); mcc_c = wave_sum(mcc_c);
  if (threadIdx.x != 0) return;
  const int it = c->iteration;
  vgg_ba_iteration li;
  li.iteration = it; li.successful = 0; li.cost = c->x_cost; li.cost_change = 0; li.gradient_max_norm = c->gmax;
  li.step_norm = 0; li.relative_decrease = 0; li.radius = c->radius;
  c->accept = 0;
  const double cand_cost = 0.5 * w.stepsum[0];
  const double mcc = w.stepsum[1] + mcc_c;         // (points' share, summed over the ranks) + (cameras' share, replicated)
  const double step_norm = sqrt(w.stepsum[2] + step_c);
  const double x_norm = sqrt(w.stepsum[3] + xn_c);
  c->cand_cost = cand_cost; c->mcc = mcc; c->step_norm = step_norm;
  const bool step_valid = !c->linear_fail && (mcc > 0.0);
  c->linear_fail = 0;
  if (!step_valid) {
    if (++c->invalid_streak >= opt.max_num_consecutive_invalid_steps) { c->done = 1; c->termination = 5; }
    c->radius /= c->decrease_factor; c->decrease_factor *= 2.0;
    c->num_unsucc += 1;
    li.radius = c->radius;
    w.log[it] = li;
    return;
  }
  c->invalid_streak = 0;
  li.step_norm = step_norm;
  li.cost_change = c->x_cost - cand_cost;
  const double ptol = opt.parameter_tolerance * (x_norm + opt.parameter_tolerance);
  if (!(step_norm > ptol)) { c->done = 1; c->termination = 3; w.log[it] = li; return; }
  if (fabs(c->x_cost - cand_cost) <= opt.function_tolerance * c->x_cost) { c->done = 1; c->termination = 2; w.log[it] = li; return; }
  const double rel = (c->x_cost - cand_cost) / mcc;
  c->rel = rel;
  li.relative_decrease = rel;
  if (rel > opt.min_relative_decrease) {
    c->accept = 1;
    c->x_cost = cand_cost;
    const double tmp = 2.0 * rel - 1.0;
    c->radius = c->radius / fmax(1.0 / 3.0, 1.0 - tmp * tmp * tmp);
    c->radius = fmin(opt.max_trust_region_radius, c->radius);
    c->decrease_factor = 2.0;
    c->need_lin = 1;
    c->num_succ += 1;
    li.successful = 1; li.cost = cand_cost;
  } else {
    c->radius /= c->decrease_factor; c->decrease_factor *= 2.0;
    c->num_unsucc += 1;
  }
  li.radius = c->radius;
  w.log[it] = li;
}

// Accepted step: the candidate becomes x, and its linearisation (cam_pass<CAND>) the one in reduce buffer 0 -- nothing is
// evaluated again at the start of the next iteration.  Rejected step: the linearisation in buffer 0 stays; with several ranks
// every rank holds its all-reduced value there, and the ranks other than 0 clear theirs, so that the SUM over the ranks
// behind the next phase 0 gives it back exactly (x + 0 + ... + 0).
__global__ void commit_kernel(Ws w, double* cam_q, double* cam_t, double* intr, double* pts, int C, int NI, int P) {
  const Ctl* ctl = w.ctl;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (!ctl->accept) {             // (accept is cleared by control_kernel on every live iteration)
    if (ctl->world > 1 && ctl->rank != 0 && i < w.lin_count) w.lin[i] = 0.0;
    return;
  }
  if (i < w.lin_count) w.lin[i] = w.lin_cand[i];
  if (i < (size_t)3 * P) pts[i] = w.cand_pts[i];
  if (i < (size_t)4 * C) cam_q[i] = w.cand_q[i];
  if (i < (size_t)3 * C) cam_t[i] = w.cand_t[i];
  if (i < (size_t)4 * NI) intr[i] = w.cand_intr[i];
}

// Overlap mode (options.overlap_factorization = number of CUs given to the factorisation, a multiple of 32; >= 2
// tile batches): two CU-masked streams split the chip while batches 1.. and the factorisation run side by side.
// Without the masks the two only overlap by accident (the tile launches fill every CU); see DESIGN.md section 6.
struct OverlapCtx {
  int chol_cus = 0;
  hipStream_t st_chol = nullptr, st_rest = nullptr;
  hipEvent_t ready = nullptr, chol_done = nullptr;
};
static OverlapCtx* overlap_ctx(const Launch& L) {
  static OverlapCtx ctx[16];
  static bool failed[16] = {};
  const int cus = L.opt.overlap_factorization;
  if (cus <= 0 || cus % 32 != 0 || L.num_batches < 2 || L.num_batches > 8 || L.num_chunks <= 0) return nullptr;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16 || failed[dev]) return nullptr;
  OverlapCtx& c = ctx[dev];
  if (c.chol_cus == cus) return &c;
  if (c.chol_cus != 0) return nullptr;             // one split per process
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess || prop.multiProcessorCount <= cus || prop.multiProcessorCount % 32 != 0) {
    failed[dev] = true; return nullptr;
  }
  const int words = prop.multiProcessorCount / 32, cw = cus / 32;
  uint32_t mask_chol[16] = {}, mask_rest[16] = {};
  if (words > 16) { failed[dev] = true; return nullptr; }
  for (int i = 0; i < words; ++i) { mask_chol[i] = (i < cw) ? 0xFFFFFFFFu : 0u; mask_rest[i] = (i < cw) ? 0u : 0xFFFFFFFFu; }
  bool ok = hipExtStreamCreateWithCUMask(&c.st_chol, words, mask_chol) == hipSuccess &&
            hipExtStreamCreateWithCUMask(&c.st_rest, words, mask_rest) == hipSuccess &&
            hipEventCreateWithFlags(&c.ready, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&c.chol_done, hipEventDisableTiming) == hipSuccess;
  if (!ok) { (void)hipGetLastError(); failed[dev] = true; return nullptr; }
  c.chol_cus = cus;
  return &c;
}

// What the host remembers about a solve between vgg_ba_begin and its phases, by workspace: whether prep_kernel still has to run
// in front of point_pass (the first linearisation: it makes scale_c), and whether every camera group has a diagonal tile
// (tile_assemble_kernel's threads are the tiles' elements: a group without observations has nobody to add its cameras' terms).
// A workspace the table does not know -- more than kHostSolves solves begun since -- takes the separate launches.
struct HostSolve { const void* ws; bool prep_pending, all_diag; };
constexpr int kHostSolves = 64;
static HostSolve g_host_solves[kHostSolves];
static int g_host_solve_next = 0;
static std::mutex g_host_solve_mutex;

static void host_solve_begin(const void* ws, bool all_diag) {
  std::lock_guard<std::mutex> lock(g_host_solve_mutex);
  HostSolve* h = nullptr;
  for (HostSolve& e : g_host_solves) if (e.ws == ws) h = &e;
  if (!h) { h = &g_host_solves[g_host_solve_next]; g_host_solve_next = (g_host_solve_next + 1) % kHostSolves; }
  *h = HostSolve{ws, true, all_diag};
}
// the entry's state; *prep_pending is handed out once
static bool host_solve_state(const void* ws, bool* prep_pending, bool* all_diag) {
  std::lock_guard<std::mutex> lock(g_host_solve_mutex);
  for (HostSolve& e : g_host_solves) {
    if (e.ws != ws || !ws) continue;
    *prep_pending = e.prep_pending; *all_diag = e.all_diag;
    e.prep_pending = false;
    return true;
  }
  return false;
}

// one copy of the tile table to the host per solve (a few hundred tiles at most), in stream order behind its upload
static bool every_group_has_diagonal_tile(const Launch& L) {
  const int G = div_up(L.d.C, kGroup);
  if (!L.tile_desc || L.num_tiles < G) return false;
  std::vector<int32_t> td((size_t)4 * L.num_tiles);
  if (hipMemcpyAsync(td.data(), L.tile_desc, sizeof(int32_t) * td.size(), hipMemcpyDeviceToHost, L.st) != hipSuccess ||
      hipStreamSynchronize(L.st) != hipSuccess) { (void)hipGetLastError(); return false; }
  std::vector<char> seen((size_t)G, 0);
  for (int t = 0; t < L.num_tiles; ++t) {
    const int gI = td[4 * t], gJ = td[4 * t + 1];
    if (gI == gJ && gI >= 0 && gI < G && td[4 * t + 3] > td[4 * t + 2]) seen[gI] = 1;
  }
  for (char c : seen) if (!c) return false;
  return true;
}

// which: 0 = the whole phase; 1 = up to the off-diagonal tile launch and the sums of its tiles; 2 = the diagonal launch, its
// sums and assemble (1 / 2: the split exchange of the sharded solve, phases 7 / 9 -- one tile batch, separate launches)
static void phase_schur(const Launch& L, int which = 0) {
  const Dims& d = L.d;
  if (which == 2) {
    if (L.num_chunks > 0) launch_schur_batches(L, 0, L.num_batches, L.st, L.w.S, nullptr, 2);
    launch_assemble(L);
    return;
  }
  // one launch for the tile sums, assembly and preparation (tile_assemble_kernel) where its conditions hold; then prep_kernel
  // runs only in front of the first point_pass of a solve
  bool prep_pending = true, all_diag = false;
  const bool known = host_solve_state(L.w.ctl, &prep_pending, &all_diag);
  const bool fused = which == 0 && known && all_diag && !g_tuning.legacy_glue && L.w.tile_rhs && L.num_chunks > 0 &&
                     L.num_batches == 1 && L.batches[3] == 0 && L.batches[4] == L.num_tiles;
  if (!fused || prep_pending) launch_prep(L);
  launch_point_pass(L);
  if (!L.w.tile_rhs) launch_cam_rhs(L);
  // (the reduced system was zeroed by cam_pass_kernel<KD, 1>: no fill launch)
  if (which == 1) {
    if (L.num_chunks > 0) launch_schur_batches(L, 0, L.num_batches, L.st, L.w.S, nullptr, 1);
    return;
  }
  if (L.num_chunks > 0) {
    if (overlap_ctx(L)) {
      // only the first batch here; the others are enqueued by phase_step beside the factorisation and land in S2
      (void)hipMemsetAsync(L.w.S2, 0, sizeof(double) * (size_t)d.n_red * d.n_red, L.st);
      launch_schur_batches(L, 0, 1, L.st, L.w.S);
    } else {
      launch_schur_batches(L, 0, L.num_batches, L.st, L.w.S, nullptr, 0, !fused);
    }
  }
  if (fused) launch_tile_assemble(L);
  else launch_assemble(L);
}

static int phase_step(const Launch& L) {
  const Dims& d = L.d;
  size_t chol_flag_count = 0;
  int32_t* chol_flags = cholesky_dataflow_flags(L.w.chol_inv, d.n_red, &chol_flag_count);
  begin_iteration_kernel<<<1, 256, 0, L.st>>>(L.w, L.opt, d.n_red, chol_flags, (int)chol_flag_count);
  int rc;
  if (OverlapCtx* oc = overlap_ctx(L)) {
    (void)hipMemsetAsync(L.w.batch_flags, 0, 64, L.st);
    (void)hipEventRecord(oc->ready, L.st);
    (void)hipStreamWaitEvent(oc->st_rest, oc->ready, 0);
    (void)hipStreamWaitEvent(oc->st_chol, oc->ready, 0);
    launch_schur_batches(L, 1, L.num_batches, oc->st_rest, L.w.S2, L.w.batch_flags);
    CholOverlap ov;
    ov.dev_flags = L.w.batch_flags + 1;            // flag of wait k = batch k + 1
    ov.S2 = L.w.S2;
    ov.first_col = 6 * kGroup * L.batches[6 * 1 + 5];
    ov.num_waits = L.num_batches - 1;
    for (int b = 1; b < L.num_batches; ++b) ov.wait_col[b - 1] = 6 * kGroup * L.batches[6 * b + 5];
    {
      ProfScope ps(kProfCholesky, oc->st_chol);
      rc = cholesky_solve_enqueue(L.w.S, L.w.rhs, d.n_red, L.w.chol_inv, &L.w.ctl->linear_fail, &L.w.ctl->done, oc->st_chol, &ov,
                                  L.chol_split_a, L.chol_split_b, L.chol_first_blk, true);
    }
    (void)hipEventRecord(oc->chol_done, oc->st_chol);
    (void)hipStreamWaitEvent(L.st, oc->chol_done, 0);
  } else {
    ProfScope ps(kProfCholesky, L.st);
    rc = cholesky_solve_enqueue(L.w.S, L.w.rhs, d.n_red, L.w.chol_inv, &L.w.ctl->linear_fail, &L.w.ctl->done, L.st, nullptr,
                                L.chol_split_a, L.chol_split_b, L.chol_first_blk, true);
  }
  if (rc != VGG_OK) return rc;
  launch_point_step(L);
  {
    // the candidate's cost and, should the step be accepted, the next linearisation (bench.py's cam_pass<linearize> slot)
    ProfScope ps(kProfLinearize, L.st);
    DevProblem dc = L.dp;
    dc.cam_q = L.w.cand_q; dc.cam_t = L.w.cand_t; dc.intr = L.w.cand_intr; dc.pts = L.w.cand_pts;
    Ws wc = L.w;
    wc.U = L.w.U_cand; wc.g = L.w.g_cand; wc.costc = L.w.cost_cand;
    launch_linearize(L, dc, wc, g_tuning.legacy_glue ? 0 : L.wgB);
  }
  if (g_tuning.legacy_glue) launch_reduce_step(L);
  return VGG_OK;
}

static void phase_update(const Launch& L) {
  const Dims& d = L.d;
  control_kernel<<<1, 64, 0, L.st>>>(L.w, L.opt, d.C);
  size_t nmax = (size_t)3 * d.P;
  if ((size_t)4 * d.C > nmax) nmax = (size_t)4 * d.C;
  if ((size_t)4 * d.NI > nmax) nmax = (size_t)4 * d.NI;
  if (L.w.lin_count > nmax) nmax = L.w.lin_count;
  commit_kernel<<<div_up((long)nmax, 256), 256, 0, L.st>>>(L.w, L.cam_q, L.cam_t, L.intr, L.pts, d.C, d.NI, d.P);
}

// compute units of the current device (256 on MI355X), looked up once per device
static int device_cus() {
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cus[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev] = n;
  }
  return cus[dev];
}

static int make_launch(const vgg_ba_problem* pb, const vgg_ba_options* opt, void* workspace, hipStream_t st, Launch* L) {
  if (!pb || !opt || !workspace) return VGG_ERR_INVALID_ARGUMENT;
  if (pb->num_cams <= 0 || pb->num_pts < 0 || pb->num_obs < 0) return VGG_ERR_INVALID_ARGUMENT;
  if (pb->num_intr != 1 && pb->num_intr != pb->num_cams) return VGG_ERR_UNSUPPORTED;
  if (pb->camera_model != kPinhole && pb->camera_model != kSimpleRadial) return VGG_ERR_UNSUPPORTED;
  L->d = make_dims(pb);
  L->dp = dev_problem(pb, L->d);
  L->w = carve(L->d, opt->max_num_iterations, pb->num_chunks, pb->num_segments, workspace);
  L->opt = *opt;
  L->st = st;
  L->lpp = lanes_per_point(L->d.P, L->d.O);
  // (every workgroup fills its LDS camera cache first: ONE resident round of the point passes -- two workgroups per CU -- is the
  //  cheapest; round 4, configs[2]: 512 workgroups point_pass + point_step 0.352 ms, 768: 0.415, 1024: 0.359, 2048: 0.371)
  L->wgB = min(max(div_up(L->d.P, 4 * (64 / L->lpp)), 1), g_tuning.point_wgs > 0 ? min(g_tuning.point_wgs, kMaxWG) : min(2 * device_cus(), kMaxWG));
  L->chunk_desc = pb->chunk_desc; L->entries = pb->entries; L->num_chunks = pb->num_chunks;
  L->merged_tile_launch = pb->merged_tile_launch;
  L->num_segments = pb->num_segments;
  L->batches = pb->tile_batches; L->num_batches = pb->num_tile_batches;
  L->chol_split_a = pb->chol_split_a; L->chol_split_b = pb->chol_split_b;
  L->chol_first_blk = pb->chol_first_blk;
  if (pb->chol_split_a < 0 || pb->chol_split_b < 0 || pb->chol_split_a % 64 != 0 ||
      pb->chol_split_a + pb->chol_split_b > 6 * pb->num_cams)
    return VGG_ERR_INVALID_ARGUMENT;
  if (pb->num_chunks > 0) {
    if (!pb->tile_batches || pb->num_tile_batches < 1) return VGG_ERR_INVALID_ARGUMENT;
    int prev_c = 0, prev_t = 0, prev_g = 0;
    for (int b = 0; b < pb->num_tile_batches; ++b) {   // consecutive, ordered ranges
      const int32_t* B = pb->tile_batches + 6 * b;
      if (B[0] != prev_c || B[1] < B[0] || B[2] < B[1] || B[3] != prev_t || B[4] < B[3] || B[5] < prev_g) return VGG_ERR_INVALID_ARGUMENT;
      prev_c = B[2]; prev_t = B[4]; prev_g = B[5];
    }
    if (prev_c != pb->num_chunks || prev_t != pb->num_tiles) return VGG_ERR_INVALID_ARGUMENT;
  }
  L->tile_desc = pb->tile_desc; L->num_tiles = pb->num_tiles;
  // reduced right-hand side from the diagonal tile launch instead of cam_pass<RHS>: compressed 6 x 6 tile blocks (shared or
  // constant intrinsics), one tile batch (the overlap mode needs the right-hand side before its later batches have run)
  // (round 6: also with per-camera intrinsics -- 7 x 7 / 8 x 8 blocks, full factors; g_tuning.tile_rhs == 1 keeps those on the
  //  camera pass, 2 = everywhere)
  L->w.tile_rhs = (g_tuning.tile_rhs && (L->d.shared || L->d.kd == 0 || g_tuning.tile_rhs >= 2) && pb->num_chunks > 0 &&
                   pb->num_tile_batches == 1) ? 1 : 0;
  L->cam_q = pb->cam_q; L->cam_t = pb->cam_t; L->intr = pb->intr; L->pts = pb->pts;
  return VGG_OK;
}

static int run_phase(const Launch& L, int phase) {
  switch (phase) {
    case 0: return VGG_OK;          // (reduce buffer 0 was filled by vgg_ba_begin or, after an accepted step, by phase 3)
    case 1: phase_schur(L); return VGG_OK;
    case 2: return phase_step(L);
    case 3: phase_update(L); return VGG_OK;
    case 4: case 5: case 6: launch_pack_lower(L, phase - 4); return VGG_OK;
    // split exchange (round 6): 7 = phase 1 up to the sums of the off-diagonal tiles, 8 = pack part A, 9 = the rest of phase 1,
    // 10 = pack part B, 11 = both parts' gathered slices -> S | rhs; 12 = "is the split available for this problem?" + the rows' offsets inside the parts (call it once per workspace)
    case 7: case 9: case 12:
      if (L.num_batches != 1 || L.merged_tile_launch || L.d.C <= kGroup) return VGG_ERR_UNSUPPORTED;   // (one camera group: no off-diagonal part)
      if (phase == 12) {                           // (also prepares the rows' offsets inside the two parts: once per workspace)
        launch_split_offsets(L);
        return VGG_OK;
      }
      phase_schur(L, phase == 7 ? 1 : 2);
      return VGG_OK;
    case 8: case 10:
      launch_pack_split(L, phase == 8 ? 0 : 1, 0);
      return VGG_OK;
    case 11:
      launch_pack_split(L, 0, 2);
      launch_pack_split(L, 1, 2);
      return VGG_OK;
    default: return VGG_ERR_INVALID_ARGUMENT;
  }
}

static int finish(const Launch& L, int max_iters, vgg_ba_summary* summary, vgg_ba_iteration* log, int log_cap) {
  Ctl h;
  if (hipMemcpyAsync(&h, L.w.ctl, sizeof(Ctl), hipMemcpyDeviceToHost, L.st) != hipSuccess) return VGG_ERR_HIP;
  int ncopy = 0;
  if (log && log_cap > 0) {
    ncopy = (max_iters + 1 < log_cap) ? max_iters + 1 : log_cap;
    if (hipMemcpyAsync(log, L.w.log, sizeof(vgg_ba_iteration) * ncopy, hipMemcpyDeviceToHost, L.st) != hipSuccess) return VGG_ERR_HIP;
  }
  if (hipStreamSynchronize(L.st) != hipSuccess) return VGG_ERR_HIP;
  if (summary) {
    summary->initial_cost = h.initial_cost; summary->final_cost = h.x_cost;
    summary->num_iterations = h.iteration; summary->num_successful_steps = h.num_succ;
    summary->num_unsuccessful_steps = h.num_unsucc; summary->termination = h.termination;
    summary->n_reduced = L.d.n_red;
    summary->num_log = (h.iteration + 1 < ncopy) ? h.iteration + 1 : ncopy;
  }
  return VGG_OK;
}

}  // namespace vgg

using namespace vgg;

extern "C" {

int vgg_ba_tuning(int lanes_per_point, int long_tracks, int cam_workgroups, int point_workgroups) {
  if (!(lanes_per_point == 0 || lanes_per_point == 8 || lanes_per_point == 16 || lanes_per_point == 32 || lanes_per_point == 64))
    return VGG_ERR_INVALID_ARGUMENT;
  vgg::g_tuning = vgg::Tuning{lanes_per_point, long_tracks < 0 ? -1 : (long_tracks ? 1 : 0), cam_workgroups > 0 ? cam_workgroups : 0,
                              point_workgroups > 0 ? point_workgroups : 0, vgg::g_tuning.tile_rhs, vgg::g_tuning.legacy_glue};
  return VGG_OK;
}

int vgg_ba_set_tile_rhs(int enable) {
  // bits 0..1: 0 / 1 / 2 as include/vggsfm_amd.h describes them; bit 2: keep the separate glue launches
  const bool known = enable >= 0 && enable <= 7 && (enable & 3) <= 2;
  vgg::g_tuning.tile_rhs = known ? (enable & 3) : 1;
  vgg::g_tuning.legacy_glue = (known && (enable & 4)) ? 1 : 0;
  return VGG_OK;
}

int vgg_ba_profile(int enable, int max_launches_per_kernel) {
  for (int k = 0; k < kProfCount; ++k) {
    for (int i = 0; i < g_prof.cap; ++i) { (void)hipEventDestroy(g_prof.start[k][i]); (void)hipEventDestroy(g_prof.stop[k][i]); }
    delete[] g_prof.start[k]; delete[] g_prof.stop[k];
    g_prof.start[k] = g_prof.stop[k] = nullptr; g_prof.n[k] = 0;
  }
  g_prof.cap = 0; g_prof.on = false;
  if (!enable) return VGG_OK;
  if (max_launches_per_kernel <= 0) return VGG_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < kProfCount; ++k) {
    g_prof.start[k] = new hipEvent_t[max_launches_per_kernel];
    g_prof.stop[k] = new hipEvent_t[max_launches_per_kernel];
    for (int i = 0; i < max_launches_per_kernel; ++i) {
      VGG_HIP_CHECK(hipEventCreate(&g_prof.start[k][i]));
      VGG_HIP_CHECK(hipEventCreate(&g_prof.stop[k][i]));
    }
  }
  g_prof.cap = max_launches_per_kernel; g_prof.on = true;
  return VGG_OK;
}

int vgg_ba_profile_read(int kernel_id, double* total_ms, int* launches, int reset) {
  if (kernel_id < 0 || kernel_id >= kProfCount || !total_ms || !launches) return VGG_ERR_INVALID_ARGUMENT;
  double tot = 0;
  for (int i = 0; i < g_prof.n[kernel_id]; ++i) {
    VGG_HIP_CHECK(hipEventSynchronize(g_prof.stop[kernel_id][i]));
    float ms = 0;
    VGG_HIP_CHECK(hipEventElapsedTime(&ms, g_prof.start[kernel_id][i], g_prof.stop[kernel_id][i]));
    tot += ms;
  }
  *total_ms = tot; *launches = g_prof.n[kernel_id];
  if (reset) g_prof.n[kernel_id] = 0;
  return VGG_OK;
}

const char* vgg_build_arch(void) { return "gfx950"; }
int vgg_abi_version(void) { return VGG_ABI_VERSION; }
size_t vgg_abi_sizeof(int which) {
  switch (which) {
    case 0: return sizeof(vgg_ba_problem);
    case 1: return sizeof(vgg_ba_options);
    case 2: return sizeof(vgg_ba_iteration);
    case 3: return sizeof(vgg_ba_summary);
    default: return 0;
  }
}

size_t vgg_ba_workspace_bytes(const vgg_ba_problem* problem, const vgg_ba_options* options) {
  if (!problem || !options) return 0;
  const Dims d = make_dims(problem);
  return carve(d, options->max_num_iterations, problem->num_chunks, problem->num_segments, nullptr).total_bytes + 256;
}

int vgg_ba_begin(const vgg_ba_problem* problem, const vgg_ba_options* options, void* workspace, size_t workspace_bytes,
                 int rank, int world_size, void* stream) {
  Launch L;
  int rc = make_launch(problem, options, workspace, (hipStream_t)stream, &L);
  if (rc != VGG_OK) return rc;
  if (workspace_bytes < L.w.total_bytes) return VGG_ERR_WORKSPACE;
  if (world_size < 1 || world_size > kPackPad || rank < 0 || rank >= world_size) return VGG_ERR_INVALID_ARGUMENT;
  host_solve_begin(L.w.ctl, L.w.tile_rhs && !g_tuning.legacy_glue && every_group_has_diagonal_tile(L));
  VGG_HIP_CHECK(hipMemsetAsync(L.w.Y, 0, L.w.y_bytes, L.st));   // absent slots stay zero for the whole solve
  // the whole S | rhs once: the phases clear and fill only the lower triangle (zero_system_lower), and nothing writes the
  // strict upper one, so it stays zero -- reduce buffer 1 as include/vggsfm_amd.h describes it
  VGG_HIP_CHECK(hipMemsetAsync(L.w.sys, 0, sizeof(double) * L.w.sys_count, L.st));
  init_kernel<<<div_up(L.d.n_red > 0 ? L.d.n_red : 1, 256), 256, 0, L.st>>>(L.dp, L.w, L.opt, rank, world_size);
  // the linearisation at the start point; every later one is cam_pass<CAND>'s of an accepted step
  launch_linearize(L, L.dp, L.w);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vgg_ba_phase(const vgg_ba_problem* problem, const vgg_ba_options* options, void* workspace, int phase, void* stream) {
  Launch L;
  int rc = make_launch(problem, options, workspace, (hipStream_t)stream, &L);
  if (rc != VGG_OK) return rc;
  rc = run_phase(L, phase);
  if (rc != VGG_OK) return rc;
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vgg_ba_reduce_buffer(const vgg_ba_problem* problem, const vgg_ba_options* options, void* workspace, int which,
                         double** device_ptr, size_t* count) {
  if (!problem || !options || !workspace || !device_ptr || !count) return VGG_ERR_INVALID_ARGUMENT;
  const Dims d = make_dims(problem);
  Ws w = carve(d, options->max_num_iterations, problem->num_chunks, problem->num_segments, workspace);
  switch (which) {
    case 0: *device_ptr = w.lin; *count = w.lin_count; break;
    case 1: *device_ptr = w.sys; *count = w.sys_count; break;
    case 2: *device_ptr = w.gmax_pts; *count = 1; break;
    case 3: *device_ptr = w.stepsum; *count = 4; break;
    case 4: *device_ptr = w.packed; *count = w.packed_count; break;
    case 5: *device_ptr = w.pk_mine; *count = w.packed_count + 2; break;
    case 6: *device_ptr = w.pk_gathered; *count = w.packed_count + 3 * kPackPad; break;
    case 7: *device_ptr = w.packed; *count = split_count_a(d); break;      // (count = elements of part A of the split exchange)
    case 8: *device_ptr = w.scale_c; *count = (size_t)d.n_red; break;      // (no reduce buffer: the Jacobi scales of the reduced columns)
    default: return VGG_ERR_INVALID_ARGUMENT;
  }
  return VGG_OK;
}

int vgg_ba_finish(const vgg_ba_problem* problem, const vgg_ba_options* options, void* workspace,
                  vgg_ba_summary* summary, vgg_ba_iteration* log, int log_cap, void* stream) {
  Launch L;
  int rc = make_launch(problem, options, workspace, (hipStream_t)stream, &L);
  if (rc != VGG_OK) return rc;
  return finish(L, options->max_num_iterations, summary, log, log_cap);
}

int vgg_ba_poll_done(const vgg_ba_problem* problem, const vgg_ba_options* options, void* workspace, int32_t* done_host,
                     void* stream) {
  if (!done_host) return VGG_ERR_INVALID_ARGUMENT;
  Launch L;
  int rc = make_launch(problem, options, workspace, (hipStream_t)stream, &L);
  if (rc != VGG_OK) return rc;
  int32_t done = 0;
  VGG_HIP_CHECK(hipMemcpyAsync(&done, &L.w.ctl->done, sizeof(done), hipMemcpyDeviceToHost, L.st));
  VGG_HIP_CHECK(hipStreamSynchronize(L.st));
  *done_host = done;
  return VGG_OK;
}

int vgg_ba_solve(const vgg_ba_problem* problem, const vgg_ba_options* options, void* workspace,
                 size_t workspace_bytes, vgg_ba_summary* summary, vgg_ba_iteration* log, int log_cap, void* stream) {
  int rc = vgg_ba_begin(problem, options, workspace, workspace_bytes, 0, 1, stream);
  if (rc != VGG_OK) return rc;
  Launch L;
  rc = make_launch(problem, options, workspace, (hipStream_t)stream, &L);
  if (rc != VGG_OK) return rc;
  // iteration max_num_iterations+1 only runs the start-of-iteration checks (gradient test after the last step).
  // Termination is decided on the device; iterations enqueued after it are no-ops, but ~100 empty launches each.
  // Every kPoll iterations the host therefore reads the `done` flag (one 4-byte copy + stream sync; the queue
  // refills within microseconds) and stops enqueuing once the solve has terminated.
  constexpr int kPoll = 8;
  for (int it = 0; it <= options->max_num_iterations; ++it) {
    for (int phase = 0; phase < 4; ++phase) {
      rc = run_phase(L, phase);
      if (rc != VGG_OK) return rc;
    }
    if (it % kPoll == kPoll - 1 && it < options->max_num_iterations) {
      int32_t done = 0;
      if (hipMemcpyAsync(&done, &L.w.ctl->done, sizeof(done), hipMemcpyDeviceToHost, L.st) != hipSuccess) return VGG_ERR_HIP;
      if (hipStreamSynchronize(L.st) != hipSuccess) return VGG_ERR_HIP;
      if (done) break;
    }
  }
  VGG_LAUNCH_CHECK();
  return finish(L, options->max_num_iterations, summary, log, log_cap);
}

}  // extern "C"
