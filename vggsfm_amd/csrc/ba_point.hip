// Bundle adjustment, the point-major launches: point_pass_kernel (per-point blocks, Schur factors), point_step_kernel
// (back-substitution, candidate points) with cam_update_kernel and reduce_step_kernel.  The driver is ba.hip.
#include "ba_obs.hpp"

namespace vgg {

#ifndef VGG_PP_ABLATE
#define VGG_PP_ABLATE 0              // profiling builds of point_pass_kernel: 1 = no Y stores, 2 = no Y sweep
#endif
#ifndef VGG_PP_OCC
#define VGG_PP_OCC 2
#endif
#ifndef VGG_PS_OCC
#define VGG_PS_OCC 2
#endif

// The split form of the point pass -- wave-per-point reductions without the Y sweep (158 VGPRs, 3 wavefronts per SIMD) +
// y_write_kernel (thread per observation, 127 VGPRs) -- was built and measured in round 2 (c3): 0.25 + 0.47 ms against
// 0.43 ms for the fused pass -- the reductions did not speed up with the third wavefront and a thread-per-observation
// writer without the LDS camera table is slower than the in-wave sweep -- so the fused pass is the one in the tree
// (DESIGN.md section 6).
// ---------------------------------------------------------------------------------------------
// point-major pass: LPP lanes per point, 64 / LPP points per wavefront (LPP = 64: one wavefront per point; 32 / 16 for
// short tracks -- the per-point work that every lane repeats (nine reductions, the 3 x 3 factorisation, ~360 of the ~640
// instructions of a point at 50 observations) is shared by 2 / 4 points, and a 12-observation track fills 12 of 16 lanes
// instead of 12 of 64).  The lanes of a point reduce among themselves (xor offsets < LPP); observations beyond the first
// LPP of a track are re-evaluated in the Y sweep.
// CY: the tile blocks are 6 x 6 (shared or constant intrinsics) and the segment buffer holds the COMPRESSED factors
// (kYc doubles per observation: N and 2 a, see y_slot_doubles); otherwise the full BD x 3 factor.
template <int KD, bool LDSCAM, bool CY, int LPP, bool LONGT = false>
__global__ __launch_bounds__(256, VGG_PP_OCC) void point_pass_kernel(DevProblem pb, Ws w, vgg_ba_options opt) {
  constexpr int BD = 6 + KD;
  __shared__ double wmax[4];
  extern __shared__ double cam_cache[];          // LDSCAM: R[9C] t[3C] pose scales[6C] flags[C] (as doubles)
  Ctl* ctl = w.ctl;
  if (ctl->done) return;
  const Dims& d = pb.d;
  constexpr int PPW = 64 / LPP;                  // points per wavefront
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int sub = lane / LPP, sl = lane % LPP;   // point of the wavefront's group, lane inside the point
  const int nw = gridDim.x * 4 * PPW;            // points per sweep of the grid
  const bool first = !ctl->scale_ready;
  const double radius = ctl->radius;
  const int kdsh = d.kdsh;
  double gmax = 0.0;
  const bool trhs = w.tile_rhs != 0;
  if (trhs) {
    // (cam_pass<RHS> is not launched: its other job -- zeroing the reduced system S | rhs for the tile sums and
    //  assemble_kernel that follow -- is done here, a few 16-byte stores per thread)
    zero_system_lower(w, pb.d.n_red, (int)blockIdx.x, (int)gridDim.x);
  }
  // shared-intrinsics terms of the reduced system that cam_pass<RHS> summed per observation (tile_rhs): they are per-POINT
  // quantities -- sum_i Ji^T E_i hs_p = Wa_p hs_p, sum_i Ji^T E_i Ms_p = Wa_p Ms_p -- added up here, one lane per point
  // (accumulators in LDS, one row per (wavefront, point slot) owned by that point's first lane: the pass has no registers to
  //  spare -- six more doubles per lane put the long-track variant on the stack)
  constexpr int KQ = (KD > 0) ? KD + KD * KD : 1;
  __shared__ double qs[4][64 / LPP][KQ];
  // compressed factors: a wavefront's 64 records of a sweep go through LDS so that SIX adjacent lanes write the six 16-byte
  // pieces of ONE record (see flush_records below)
  __shared__ __attribute__((aligned(16))) double2 ystage[CY ? 4 : 1][CY ? 64 * (kYc / 2) : 1];
  __shared__ int32_t slotstage[CY ? 4 : 1][CY ? 64 : 1];
  if (trhs && KD > 0 && (lane % LPP) == 0) {
#pragma unroll
    for (int i = 0; i < KQ; ++i) qs[wave][lane / LPP][i] = 0.0;
  }
  // The per-observation camera gather is the second of three dependent memory round trips of a point; with the
  // cameras in LDS it is an LDS read.  (The wavefronts are latency bound: SQ_WAIT_ANY 60 %, 2 waves/SIMD.)
  const double* lq = cam_cache;                  // rotation matrices [9C]
  const double* lt = lq + 9 * d.C;
  const double* lsc = lt + 3 * d.C;
  const double* lfl = lsc + 6 * d.C;
  if (LDSCAM) {
    for (int i = threadIdx.x; i < d.C; i += 256) {
      quat_to_R(pb.cam_q + 4 * i, cam_cache + 9 * i);
      cam_cache[18 * d.C + i] = pb.cam_const ? (double)pb.cam_const[i] : 0.0;
    }
    for (int i = threadIdx.x; i < 3 * d.C; i += 256) cam_cache[9 * d.C + i] = pb.cam_t[i];
    for (int i = threadIdx.x; i < 6 * d.C; i += 256) cam_cache[12 * d.C + i] = w.scale_c[i];
    __syncthreads();
  }
  // software pipeline over the points of this wavefront: the row bounds / coordinates of the NEXT point and the
  // camera index, pixel and slot of its first 64 observations are loaded while the current point is processed
  int p = (blockIdx.x * 4 + wave) * PPW + sub;   // (the lanes of one point run the same control flow: per-lane loops below)
  // (camera, pixel, slot) of the lane's first NPF observations (o0 + sl + k LPP) are prefetched with the point; later
  // ones are loaded where they are used
  // LONGT (tracks of several sweeps: mean length > 1.5 LPP): four observations per lane prefetched and NO cached Jacobians
  // (the cache serves one sweep in four there and costs 36 registers) -- every load of a point is then issued before the
  // Y stores of the previous one (loads issued behind a burst of stores wait for the stores' acknowledgements)
  constexpr int NPF = LONGT ? 4 : 2;
  constexpr bool CACHEJ = !LONGT;
  int n_o0 = 0, n_o1 = 0;
  ObsPf<NPF> n_pf;
  double n_X0 = 0, n_X1 = 0, n_X2 = 0;
  int n_ptc = 0;                                // (constant-point flag as loaded: tested where it is used -- a test right
                                                //  behind the load is a wait for it, and for every load issued before it)
  // (two stages: the row bounds / coordinates are loaded TWO points ahead, the observations ONE point ahead, so
  //  that the observation loads never wait for the row-bound load they depend on)
  int m_o0 = 0, m_o1 = 0;
  double m_X0 = 0, m_X1 = 0, m_X2 = 0;
  int m_ptc = 0;
  if (p < d.P) {
    n_o0 = pb.row_ptr[p]; n_o1 = pb.row_ptr[p + 1];
    n_X0 = pb.pts[3 * p]; n_X1 = pb.pts[3 * p + 1]; n_X2 = pb.pts[3 * p + 2];
    n_ptc = pb.pt_const ? (int)pb.pt_const[p] : 0;
    n_pf.template load<true>(pb.obs_cam, pb.obs_uv, pb.obs_slot, n_o0, n_o1, LPP, sl);
    if (p + nw < d.P) {
      const int pm = p + nw;
      m_o0 = pb.row_ptr[pm]; m_o1 = pb.row_ptr[pm + 1];
      m_X0 = pb.pts[3 * pm]; m_X1 = pb.pts[3 * pm + 1]; m_X2 = pb.pts[3 * pm + 2];
      m_ptc = pb.pt_const ? (int)pb.pt_const[pm] : 0;
    }
  }
  // (compressed factors: the loop is WAVE-uniform -- the record flush below needs all 64 lanes; a lane group whose point index
  //  has run past the end goes through a last trip with an empty point: o0 = o1 = 0, nothing read or written for it)
  for (; CY ? __any(p < d.P) : (p < d.P); p += nw) {
    const bool pvalid = p < d.P;
    const int o0 = pvalid ? n_o0 : 0, o1 = pvalid ? n_o1 : 0;
    const double X[3] = {n_X0, n_X1, n_X2};
    const bool pt_c = n_ptc != 0;
    const ObsPf<NPF> f_pf = n_pf;
    {
      // stage 1 -> current of the next iteration: observations of point p + nw (its bounds arrived an iteration ago)
      n_o0 = m_o0; n_o1 = m_o1; n_X0 = m_X0; n_X1 = m_X1; n_X2 = m_X2; n_ptc = m_ptc;
      if (p + nw < d.P) n_pf.template load<true>(pb.obs_cam, pb.obs_uv, pb.obs_slot, n_o0, n_o1, LPP, sl);
      // stage 2: bounds / coordinates of point p + 2 nw
      const int pm = p + 2 * nw;
      if (pm < d.P) {
        m_o0 = pb.row_ptr[pm]; m_o1 = pb.row_ptr[pm + 1];
        m_X0 = pb.pts[3 * pm]; m_X1 = pb.pts[3 * pm + 1]; m_X2 = pb.pts[3 * pm + 2];
        m_ptc = pb.pt_const ? (int)pb.pt_const[pm] : 0;
      }
    }
    double V[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0}, Wa[3 * (KD ? KD : 1)];
#pragma unroll
    for (int i = 0; i < 3 * (KD ? KD : 1); ++i) Wa[i] = 0;
    // (the point's Jacobi scales are requested in front of the sweep that hides their round trip, not behind it)
    double sp[3] = {1.0, 1.0, 1.0};
    if (!first && pvalid) { sp[0] = w.scale_p[3 * (size_t)p]; sp[1] = w.scale_p[3 * (size_t)p + 1]; sp[2] = w.scale_p[3 * (size_t)p + 2]; }
    // Jacobians of this lane's first observation for the Y sweep (tracks > LPP recompute): F and E, or -- compressed
    // factors -- the 2 x 3 d r / d (R X + t) instead of F
    double cF[CY ? 6 : 2 * BD], cE[6];
    // compressed factors (round 3): the 2 x 3 d r / d (R X + t) of the lane's first NPF observations is kept for the Y sweep,
    // which then needs no second evaluation (E = Jw R, a = R X from the camera table); the sweeps are unrolled over those
    // slices so that the kept values sit in registers; longer tracks re-evaluate the rest
    constexpr bool KEEPJ = CY;
    double cJ[KEEPJ ? NPF : 1][6];
    auto sweep1 = [&](const int pass, const int o, double* keepJ) __attribute__((always_inline)) {
      const bool head = pass == 0;
      const int c = f_pf.cam(pass, pb.obs_cam, o);
      const float2 uv = f_pf.uv(pass, pb.obs_uv, o);
      const int a = d.shared ? 0 : c;
      double r[2], F[2 * BD], E[6], Jw[6];
      if (LDSCAM)
        eval_full<KD>(d, lq + 9 * c, lt + 3 * c, pb.intr + 4 * a, X, uv, (unsigned)lfl[c],
                      pb.intr_const ? pb.intr_const[a] != 0 : false, pt_c, r, F, E, CY ? Jw : nullptr);
      else
        eval_full<KD>(d, CamR(pb.cam_q + 4 * c).R, pb.cam_t + 3 * c, pb.intr + 4 * a, X, uv,
                      pb.cam_const ? pb.cam_const[c] : 0u, pb.intr_const ? pb.intr_const[a] != 0 : false, pt_c, r, F, E,
                      CY ? Jw : nullptr);
      if (CACHEJ && !KEEPJ && head) {
#pragma unroll
        for (int i = 0; i < (CY ? 6 : 2 * BD); ++i) cF[i] = CY ? Jw[i] : F[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) cE[i] = E[i];
      }
      if (KEEPJ && keepJ) {
#pragma unroll
        for (int i = 0; i < 6; ++i) keepJ[i] = Jw[i];
      }
      V[0] += E[0] * E[0] + E[3] * E[3]; V[1] += E[0] * E[1] + E[3] * E[4]; V[2] += E[0] * E[2] + E[3] * E[5];
      V[3] += E[1] * E[1] + E[4] * E[4]; V[4] += E[1] * E[2] + E[4] * E[5]; V[5] += E[2] * E[2] + E[5] * E[5];
      g[0] += E[0] * r[0] + E[3] * r[1]; g[1] += E[1] * r[0] + E[4] * r[1]; g[2] += E[2] * r[0] + E[5] * r[1];
      if (KD > 0 && kdsh) {
#pragma unroll
        for (int m = 0; m < KD; ++m)
#pragma unroll
          for (int b = 0; b < 3; ++b) Wa[m * 3 + b] += F[6 + m] * E[b] + F[BD + 6 + m] * E[3 + b];
      }
    };
    if constexpr (KEEPJ) {
#pragma unroll
      for (int ps = 0; ps < NPF; ++ps) {
        const int o = o0 + sl + ps * LPP;
        if (o < o1) sweep1(ps, o, cJ[ps]);
      }
      for (int o = o0 + sl + NPF * LPP; o < o1; o += LPP) sweep1((o - o0) / LPP, o, nullptr);
    } else {
      for (int o = o0 + sl; o < o1; o += LPP) sweep1((o - o0) / LPP, o, nullptr);
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) V[i] = group_sum<LPP>(V[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) g[i] = group_sum<LPP>(g[i]);
    if (KD > 0 && kdsh) {
#pragma unroll
      for (int i = 0; i < 3 * KD; ++i) Wa[i] = group_sum<LPP>(Wa[i]);
    }
    // every lane of the point now holds the totals; its lane 0 writes
    double s[3];
    const double colsq[3] = {V[0], V[3], V[5]};
    if (first) {
#pragma unroll
      for (int k = 0; k < 3; ++k) s[k] = opt.jacobi_scaling ? 1.0 / (1.0 + sqrt(colsq[k])) : 1.0;
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) s[k] = sp[k];
    }
    double Gm[6] = {0, 0, 0, 0, 0, 0}, hs[3] = {0, 0, 0}, pd[3] = {0, 0, 0};
    double Ms[3 * (KD ? KD : 1)];
#pragma unroll
    for (int i = 0; i < 3 * (KD ? KD : 1); ++i) Ms[i] = 0;
    bool z_written = false;                           // tile_rhs: Z = [z | y_0 | y_1] with hs = G z, Ms_m = G y_m
    if (!pt_c && o1 > o0) {
      double dd[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) dd[k] = fmin(fmax(colsq[k] * s[k] * s[k], opt.min_lm_diagonal), opt.max_lm_diagonal) / radius;
#pragma unroll
      for (int k = 0; k < 3; ++k) pd[k] = dd[k] / (s[k] * s[k]);
      const double a00 = V[0] * s[0] * s[0] + dd[0], a10 = V[1] * s[0] * s[1], a20 = V[2] * s[0] * s[2];
      const double a11 = V[3] * s[1] * s[1] + dd[1], a21 = V[4] * s[1] * s[2], a22 = V[5] * s[2] * s[2] + dd[2];
      bool ok = a00 > 0;
      const double l00 = sqrt(a00);
      const double l10 = a10 / l00, l20 = a20 / l00;
      const double d11 = a11 - l10 * l10;
      ok = ok && d11 > 0;
      const double l11 = sqrt(d11);
      const double l21 = (a21 - l20 * l10) / l11;
      const double d22 = a22 - l20 * l20 - l21 * l21;
      ok = ok && d22 > 0;
      const double l22 = sqrt(d22);
      if (!ok) { if (sl == 0) ctl->linear_fail = 1; }
      // Linv (lower): i00 i10 i11 i20 i21 i22
      // (measured, round 4: reciprocal square roots + Newton steps instead of sqrt and the six IEEE divisions -- a third of
      //  the dependent instructions of this per-point chain -- change nothing in the launch time; the oracle's arithmetic stays)
      const double i00 = 1 / l00, i11 = 1 / l11, i22 = 1 / l22;
      const double i10 = -l10 * i00 * i11;
      const double i21 = -l21 * i11 * i22;
      const double i20 = -(l20 * i00 + l21 * i10) * i22;
      // G = S_p * Linv^T (upper triangular): G[b][m], b <= m   stored as G00 G01 G02 G11 G12 G22
      Gm[0] = s[0] * i00; Gm[1] = s[0] * i10; Gm[2] = s[0] * i20; Gm[3] = s[1] * i11; Gm[4] = s[1] * i21; Gm[5] = s[2] * i22;
      // z = Linv * (s o g) ; hs = G z
      const double gs0 = s[0] * g[0], gs1 = s[1] * g[1], gs2 = s[2] * g[2];
      const double z0 = i00 * gs0, z1 = i10 * gs0 + i11 * gs1, z2 = i20 * gs0 + i21 * gs1 + i22 * gs2;
      hs[0] = Gm[0] * z0 + Gm[1] * z1 + Gm[2] * z2; hs[1] = Gm[3] * z1 + Gm[4] * z2; hs[2] = Gm[5] * z2;
      if (trhs && sl == 0) {
        double* Z = w.Zp + 9 * (size_t)p;
        Z[0] = z0; Z[1] = z1; Z[2] = z2;
        if (KD == 0) { Z[3] = 0; Z[4] = 0; Z[5] = 0; Z[6] = 0; Z[7] = 0; Z[8] = 0; }   // (KD > 0, per-camera intrinsics: the full-factor tiles read z only)
        if (KD == 1 && kdsh) { Z[6] = 0; Z[7] = 0; Z[8] = 0; }
      }
      z_written = true;
      if (KD > 0 && kdsh) {
#pragma unroll
        for (int m = 0; m < KD; ++m) {
          const double sa = w.scale_c[6 * d.C + m];
          // W_a (scaled) row m: sa * Wa[m][b] * s[b];  Ms[:,m] = G G^T (S_p^-1 ...)  -> S_p V^-1 W_a^T = G (Linv (s o Wa^T)) * sa
          const double w0 = sa * s[0] * Wa[m * 3], w1 = sa * s[1] * Wa[m * 3 + 1], w2 = sa * s[2] * Wa[m * 3 + 2];
          const double y0 = i00 * w0, y1 = i10 * w0 + i11 * w1, y2 = i20 * w0 + i21 * w1 + i22 * w2;
          Ms[m * 3] = Gm[0] * y0 + Gm[1] * y1 + Gm[2] * y2; Ms[m * 3 + 1] = Gm[3] * y1 + Gm[4] * y2; Ms[m * 3 + 2] = Gm[5] * y2;
          if (trhs && sl == 0) { double* Z = w.Zp + 9 * (size_t)p + 3 + 3 * m; Z[0] = y0; Z[1] = y1; Z[2] = y2; }
        }
        if (trhs && sl == 0) {
          double* q = qs[wave][sub];
#pragma unroll
          for (int i = 0; i < KD; ++i) {
            q[i] += Wa[i * 3] * hs[0] + Wa[i * 3 + 1] * hs[1] + Wa[i * 3 + 2] * hs[2];
#pragma unroll
            for (int j = 0; j < KD; ++j)
              q[KD + i * KD + j] += Wa[i * 3] * Ms[j * 3] + Wa[i * 3 + 1] * Ms[j * 3 + 1] + Wa[i * 3 + 2] * Ms[j * 3 + 2];
          }
        }
      }
      gmax = fmax(gmax, fmax(fabs(g[0]), fmax(fabs(g[1]), fabs(g[2]))));
    }
    // per-observation Schur factors Y_i = s_c o ((F_i^T E_i) G) -> slot obs_slot[o] of the zero-padded
    // segment buffer consumed by schur_tile_kernel
    if (VGG_PP_ABLATE != 2) {
      const int bdt = d.shared ? 6 : BD;          // rows of the tile block (intrinsics only when per camera)
      auto emit = [&](const int pass, const int o, const double* keptJ) __attribute__((always_inline)) {
        const bool head = pass == 0;
        const int c = f_pf.cam(pass, pb.obs_cam, o);
        double F[CY ? 6 : 2 * BD], E[6];          // (CY: F holds the 2 x 3 Jw)
        if (KEEPJ && keptJ) {                     // kept from the first sweep: E = Jw R as obs_eval_R forms it
          double Rl[9];
          const double* Rc = Rl;
          if (LDSCAM) Rc = lq + 9 * c; else quat_to_R(pb.cam_q + 4 * c, Rl);
#pragma unroll
          for (int i = 0; i < 6; ++i) F[i] = keptJ[i];
#pragma unroll
          for (int row = 0; row < 2; ++row)
#pragma unroll
            for (int k = 0; k < 3; ++k)
              E[3 * row + k] = pt_c ? 0.0 : keptJ[3 * row] * Rc[k] + keptJ[3 * row + 1] * Rc[3 + k] + keptJ[3 * row + 2] * Rc[6 + k];
        } else if (CACHEJ && !KEEPJ && head) {    // cached Jacobians of the first slice
#pragma unroll
          for (int i = 0; i < (CY ? 6 : 2 * BD); ++i) F[i] = cF[i];
#pragma unroll
          for (int i = 0; i < 6; ++i) E[i] = cE[i];
        } else {
          const int a = d.shared ? 0 : c;
          double r[2], Ff[2 * BD];
          const float2 uv = f_pf.uv(pass, pb.obs_uv, o);
          if (LDSCAM)
            eval_full<KD>(d, lq + 9 * c, lt + 3 * c, pb.intr + 4 * a, X, uv, (unsigned)lfl[c],
                          pb.intr_const ? pb.intr_const[a] != 0 : false, pt_c, r, CY ? Ff : F, E, CY ? F : nullptr);
          else
            eval_full<KD>(d, CamR(pb.cam_q + 4 * c).R, pb.cam_t + 3 * c, pb.intr + 4 * a, X, uv,
                          pb.cam_const ? pb.cam_const[c] : 0u, pb.intr_const ? pb.intr_const[a] != 0 : false, pt_c, r,
                          CY ? Ff : F, E, CY ? F : nullptr);
        }
        const int slot = f_pf.slot(pass, pb.obs_slot, o);
        if constexpr (CY) {
          // compressed factor: N = Jw^T (E G) (3 x 3, row-major) and 2 a = 2 R X -- one run of 96 bytes per observation
          double M[6];
          M[0] = E[0] * Gm[0]; M[1] = E[0] * Gm[1] + E[1] * Gm[3]; M[2] = E[0] * Gm[2] + E[1] * Gm[4] + E[2] * Gm[5];
          M[3] = E[3] * Gm[0]; M[4] = E[3] * Gm[1] + E[4] * Gm[3]; M[5] = E[3] * Gm[2] + E[4] * Gm[4] + E[5] * Gm[5];
          double rec[kYc];
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int m = 0; m < 3; ++m) rec[3 * i + m] = F[i] * M[m] + F[3 + i] * M[3 + m];
          double Rl[9];
          const double* Rc = Rl;
          if (LDSCAM) Rc = lq + 9 * c; else quat_to_R(pb.cam_q + 4 * c, Rl);
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            const double ai = Rc[3 * i] * X[0] + Rc[3 * i + 1] * X[1] + Rc[3 * i + 2] * X[2];
            rec[9 + i] = ai + ai;
          }
          // (into the wavefront's LDS image, row = lane; flush_records writes it out)
          slotstage[wave][lane] = slot;
#pragma unroll
          for (int i = 0; i < kYc / 2; ++i) ystage[wave][lane * (kYc / 2) + i] = make_double2(rec[2 * i], rec[2 * i + 1]);
        } else {
        // segment layout: [component 0..2][slot 0..15][row 0..bdt-1]  (three rows of the K dimension)
        const int rt = kGroup * bdt;
        double* y = w.Y + (size_t)(slot >> 4) * (3 * rt) + (slot & 15) * bdt;
        // the lane's three runs of bdt doubles go out 16 bytes at a time when bdt is even (the runs are then 16-byte
        // aligned): half the store instructions and half the partial-line transactions of 8-byte stores.
        const bool pairs = (bdt & 1) == 0;
        double prev[3] = {0, 0, 0};
#pragma unroll
        for (int i = 0; i < BD; ++i) {
          if (i < bdt) {
            const double sc = (i < 6) ? (LDSCAM ? lsc[6 * c + i] : w.scale_c[6 * c + i])
                                      : w.scale_c[6 * d.C + KD * c + (i - 6)];
            const double w0 = F[i] * E[0] + F[BD + i] * E[3], w1 = F[i] * E[1] + F[BD + i] * E[4],
                         w2 = F[i] * E[2] + F[BD + i] * E[5];
            const double y0 = sc * (w0 * Gm[0]), y1 = sc * (w0 * Gm[1] + w1 * Gm[3]), y2 = sc * (w0 * Gm[2] + w1 * Gm[4] + w2 * Gm[5]);
#if VGG_PP_ABLATE == 1                            // profiling build: the Y arithmetic without its stores
            if (Gm[0] == 12345.678) {
#endif
            if (!pairs) { y[i] = y0; y[rt + i] = y1; y[2 * rt + i] = y2; }
            else if (i & 1) {
              *reinterpret_cast<double2*>(y + i - 1) = make_double2(prev[0], y0);
              *reinterpret_cast<double2*>(y + rt + i - 1) = make_double2(prev[1], y1);
              *reinterpret_cast<double2*>(y + 2 * rt + i - 1) = make_double2(prev[2], y2);
            } else { prev[0] = y0; prev[1] = y1; prev[2] = y2; }
#if VGG_PP_ABLATE == 1
            }
#endif
          }
        }
        }
      };
      if constexpr (KEEPJ) {
        // A sweep's records leave the wavefront through LDS: lane q of store k carries piece (k 64 + q) % 6 of record
        // (k 64 + q) / 6, so six adjacent lanes cover one 96-byte record and a store instruction touches ~16 cache-line
        // sectors instead of 64.  (Lane = record, six 16-byte stores per lane: every store was its own L2 transaction,
        // 30 M per launch at configs[2].  Ablations: the launch without these stores 0.152 ms, without the whole sweep
        // 0.117, with them 0.249; this form 0.244 against 0.262 on the same box, profiles/r04_ab_point_pass_records.jsonl --
        // what is left of the stores' cost is their 0.5 GB at the HBM write rate.)  In-order LDS per wavefront: no barrier.
        auto flush_records = [&]() __attribute__((always_inline)) {
#if VGG_PP_ABLATE != 1                            // (profiling build 1: the Y arithmetic without its stores)
#pragma unroll
          for (int k = 0; k < kYc / 2; ++k) {
            const int q = k * 64 + lane;
            const int r = (q * 10923) >> 16;        // q / 6 for q < 384
            const int pc = q - 6 * r;
            const int sdst = slotstage[wave][r];
            const double2 v = ystage[wave][q];
            if (sdst >= 0) reinterpret_cast<double2*>(w.Y)[(size_t)sdst * (kYc / 2) + pc] = v;
          }
#endif
        };
#pragma unroll
        for (int ps = 0; ps < NPF; ++ps) {
          const int o = o0 + sl + ps * LPP;
          if (!__any(o < o1)) break;
          if (o < o1) emit(ps, o, cJ[ps]); else slotstage[wave][lane] = -1;
          flush_records();
        }
        for (int pass = NPF; __any(o0 + sl + pass * LPP < o1); ++pass) {
          const int o = o0 + sl + pass * LPP;
          if (o < o1) emit(pass, o, nullptr); else slotstage[wave][lane] = -1;
          flush_records();
        }
      } else {
        for (int o = o0 + sl; o < o1; o += LPP) emit((o - o0) / LPP, o, nullptr);
      }
    }
    if (sl == 0 && pvalid) {
      if (first) { w.scale_p[3 * p] = s[0]; w.scale_p[3 * p + 1] = s[1]; w.scale_p[3 * p + 2] = s[2]; }
#pragma unroll
      for (int i = 0; i < 6; ++i) w.G[6 * (size_t)p + i] = Gm[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) { w.hs[3 * (size_t)p + i] = hs[i]; w.pdamp[3 * (size_t)p + i] = pd[i]; }
      if (KD > 0 && kdsh) {
#pragma unroll
        for (int i = 0; i < 3 * KD; ++i) w.Ms[(size_t)p * 3 * kdsh + i] = Ms[i];
      }
      if (trhs && !z_written) {                       // constant / unobserved point: no step, no contribution
#pragma unroll
        for (int i = 0; i < 9; ++i) w.Zp[9 * (size_t)p + i] = 0.0;
      }
    }
  }
  gmax = wave_max(gmax);
  if (lane == 0) wmax[wave] = gmax;
  __syncthreads();
  if (threadIdx.x == 0) w.part_B[blockIdx.x] = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
  if (trhs && KD > 0) {
    __syncthreads();                                  // (every slot's owner lane has finished its points)
    if (threadIdx.x < KQ) {
      double v = 0.0;                                 // fixed order: wavefront, then point slot
      for (int wv = 0; wv < 4; ++wv)
        for (int sb = 0; sb < 64 / LPP; ++sb) v += qs[wv][sb][threadIdx.x];
      w.part_Q[8 * blockIdx.x + threadIdx.x] = v;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// candidate cameras: x (+) (-s o y); also the camera-side part of |step| and |x| and, with CAM_MCC, the cameras' share of the
// model cost change.  One thread per camera c < C and one more (c == C) for a shared intrinsics block.
//
// The cameras' share: with m = -(F dy + E ys) the model residual of an observation, the terms of -sum m.(r + m/2) that hold
// dy alone are sum_obs [F dy . r - |F dy|^2 / 2] (see point_step_kernel).  Summed camera by camera they are
//   dy_c^T g_c - dy_c^T U_c dy_c / 2,      g_c = sum F^T r,  U_c = sum F^T F  (dy_c: the six pose entries, then the intrinsics')
// -- the linearisation cam_pass<.,0> stored in reduce buffer 0 at this very point (corrected, constant-masked, unscaled; with
// several ranks all-reduced, so the share is the same on every rank and control_kernel adds it un-reduced).  A shared
// intrinsics block enters through every camera's BD x BD block.
template <int KD>
__device__ __forceinline__ void cam_update_body(const DevProblem& pb, const Ws& w, int c) {
  constexpr int BD = 6 + KD;
  const Dims& d = pb.d;
  double step = 0, xn = 0, mcc = 0;
  if (c < d.C) {
    double dl[6], dyc[BD];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int j = 6 * c + k;
      const double dyv = w.active[j] ? w.scale_c[j] * w.rhs[j] : 0.0;
      w.dy[j] = dyv;
      dyc[k] = dyv;
      dl[k] = -dyv;
    }
    double qn[4];
    quat_plus_select(pb.cam_q + 4 * c, dl, qn);
    // |x| counts only blocks Ceres keeps in the reduced program (a constant pose is removed from it)
    const bool pose_var = !(pb.cam_const && (pb.cam_const[c] & 1u));
#pragma unroll
    for (int k = 0; k < 4; ++k) { w.cand_q[4 * c + k] = qn[k]; const double df = qn[k] - pb.cam_q[4 * c + k]; step += df * df; if (pose_var) xn += pb.cam_q[4 * c + k] * pb.cam_q[4 * c + k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) { const double tn = pb.cam_t[3 * c + k] + dl[3 + k]; w.cand_t[3 * c + k] = tn; step += dl[3 + k] * dl[3 + k]; if (pose_var) xn += pb.cam_t[3 * c + k] * pb.cam_t[3 * c + k]; }
#pragma unroll
    for (int k = 0; k < KD; ++k) {
      const int j = 6 * d.C + KD * (d.shared ? 0 : c) + k;
      dyc[6 + k] = w.active[j] ? w.scale_c[j] * w.rhs[j] : 0.0;
    }
    const double* U = w.U + (size_t)c * BD * BD;
    const double* g = w.g + (size_t)c * BD;
    double lin = 0, quad = 0;
#pragma unroll
    for (int i = 0; i < BD; ++i) {
      double ud = 0;
#pragma unroll
      for (int k = 0; k < BD; ++k) ud += U[i * BD + k] * dyc[k];
      lin += dyc[i] * g[i];
      quad += dyc[i] * ud;
    }
    mcc = lin - 0.5 * quad;
  }
  // intrinsics block a == c (per camera) or block 0 handled by the extra thread c == C (shared)
  const int a = d.shared ? ((c == d.C) ? 0 : -1) : ((c < d.C) ? c : -1);
  if (a >= 0) {
    // (statically indexed throughout: an array indexed by a run-time slot is a stack object, and point_step_kernel, which
    //  runs this body in its prologue, has no scratch)
    double in4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) in4[k] = pb.intr[4 * a + k];
#pragma unroll
    for (int k = 0; k < KD; ++k) {
      const int j = 6 * d.C + KD * a + k;
      const double dyv = w.active[j] ? w.scale_c[j] * w.rhs[j] : 0.0;
      w.dy[j] = dyv;
      const bool extra = (KD == 2) ? (k == 1) : (d.only_k != 0);    // the entry steps k (slot 3), else f (slot 0)
      if (extra) in4[3] -= dyv; else in4[0] -= dyv;
      step += dyv * dyv;
    }
    const bool intr_var = KD > 0 && !(pb.intr_const && pb.intr_const[a]);
    const int np = (d.model == kSimpleRadial) ? 4 : 3;
#pragma unroll
    for (int k = 0; k < 4; ++k) { w.cand_intr[4 * a + k] = in4[k]; if (intr_var && k < np) xn += pb.intr[4 * a + k] * pb.intr[4 * a + k]; }
  }
  w.cam_part[3 * c] = step;
  w.cam_part[3 * c + 1] = xn;
  w.cam_part[3 * c + 2] = mcc;
}

// (a launch of its own where point_step_kernel does not run the body in its prologue: a camera table over 64 KB, the
//  separate glue launches)
template <int KD>
__global__ void cam_update_kernel(DevProblem pb, Ws w) {
  if (w.ctl->done) return;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > pb.d.C) return;
  cam_update_body<KD>(pb, w, c);
}

// back-substitution, model cost change and candidate point: LPP lanes per point (see point_pass_kernel).  The candidate's
// cost is not evaluated here: cam_pass<CAND> behind this launch evaluates the candidate's residuals with their Jacobians, and
// its cost decides the step.  (A second sweep here used to evaluate the same residuals for the cost alone, and after an
// accepted step cam_pass<LIN> evaluated them once more; c3: this launch 0.101 -> 0.079 ms without that sweep.)
//
// The sweep is in directional form.  What it needs of an observation is fy = F dy_c -- ONE directional derivative along the
// camera's step -- and the adjoint product E^T fy = R^T JY^T fy, so neither the 2 x BD block F nor the 2 x 3 block E is built
// (obs_step_R, camera_model.hpp).  dy is zero in every inactive column (cam_update_body; init_kernel derives `active` from
// cam_const / intr_const exactly as eval_full masks F), so the constant-parameter masks of F drop out; a constant point
// contributes nothing, as E = 0 did.  The cameras' share of the model cost change comes from cam_update_body, camera by
// camera from U | g, so under the trivial loss the sweep needs no residual at all.  Robust loss (kernel-uniform branch):
// the corrector C = sqrt(rho') (I - alpha r r^T) multiplies both Jacobians from the left, fy' = C fy and E'^T fy' = E^T C fy'.
// (The sweep over full Jacobians it replaced: tests/test_gpu_ba_step_sweep.py, profiles/r09_port_deviation_*.txt.)
//
// fused (LDSCAM only): no cam_update launch in front.  Every workgroup fills its LDS table of dy from active / scale_c / rhs
// -- the sweep reads NO w.dy from global memory, which another workgroup of this launch may not have written yet -- and the
// LAST workgroup (one per 256 cameras) runs cam_update_body, a thread per camera (w.dy, the candidate cameras, cam_part: read
// by later launches only).  The last ones because their wavefronts have the fewest points when P is no multiple of the
// launch's stride.
template <int KD, bool LDSCAM, int LPP, bool LONGT = false>
__global__ __launch_bounds__(256, VGG_PS_OCC) void point_step_kernel(DevProblem pb, Ws w, int fused) {
  __shared__ double red[4][3];
  extern __shared__ double cam_cache[];   // LDSCAM: R[9C] t[3C] dy[6C + KD NI = n_red]
  if (w.ctl->done) return;
  const Dims& d = pb.d;
  constexpr int PPW = 64 / LPP;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int sub = lane / LPP, sl = lane % LPP;
  const int nw = gridDim.x * 4 * PPW;
  double s_mcc = 0, s_step = 0, s_xn = 0;
  const double* lq = cam_cache;                  // rotation matrices [9C]
  const double* lt = lq + 9 * d.C;
  const double* ldy = lt + 3 * d.C;
  const double* ldi = ldy + 6 * d.C;              // the intrinsics entries of dy [KD NI]
  if (LDSCAM) {
    double* cc = cam_cache;
    for (int i = threadIdx.x; i < d.C; i += 256) quat_to_R(pb.cam_q + 4 * i, cc + 9 * i);
    for (int i = threadIdx.x; i < 3 * d.C; i += 256) cc[9 * d.C + i] = pb.cam_t[i];
    // dy: the poses' entries first, then the intrinsics', as in w.dy
    if (fused) {
      // (the products cam_update_body stores in w.dy, made here from the same operands: the same bits; unrolled so that
      //  the loads of four entries are in flight together -- 3200 entries at 400 cameras with their own intrinsics)
#pragma unroll 4
      for (int i = threadIdx.x; i < d.n_red; i += 256) cc[12 * d.C + i] = w.active[i] ? w.scale_c[i] * w.rhs[i] : 0.0;
      // the last ceil((C + 1) / 256) workgroups take 256 cameras each (fewer workgroups than that: they take turns)
      const int nbody = min((int)gridDim.x, (d.C + 256) / 256);
      const int jb = (int)gridDim.x - 1 - (int)blockIdx.x;
      if (jb < nbody) {
        for (int c = jb * 256 + threadIdx.x; c <= d.C; c += 256 * nbody) cam_update_body<KD>(pb, w, c);
        if (jb == 0 && threadIdx.x == 0) w.ctl->fused_step_prologues += 1;
      }
    } else {
#pragma unroll 4
      for (int i = threadIdx.x; i < d.n_red; i += 256) cc[12 * d.C + i] = w.dy[i];
    }
    __syncthreads();
  }
  (void)ldi;
  // same software pipeline over the points of a wavefront as in point_pass_kernel
  int p = (blockIdx.x * 4 + wave) * PPW + sub;
  constexpr int NPF = LONGT ? 4 : 2;             // prefetched observations per lane (see point_pass_kernel)
  int n_o0 = 0, n_o1 = 0;
  ObsPf<NPF> n_pf;
  double n_X0 = 0, n_X1 = 0, n_X2 = 0;
  int n_ptc = 0;                                // (constant-point flag as loaded: tested where it is used -- a test right
                                                //  behind the load is a wait for it, and for every load issued before it)
  // (two stages: the row bounds / coordinates are loaded TWO points ahead, the observations ONE point ahead, so
  //  that the observation loads never wait for the row-bound load they depend on)
  int m_o0 = 0, m_o1 = 0;
  double m_X0 = 0, m_X1 = 0, m_X2 = 0;
  int m_ptc = 0;
  if (p < d.P) {
    n_o0 = pb.row_ptr[p]; n_o1 = pb.row_ptr[p + 1];
    n_X0 = pb.pts[3 * p]; n_X1 = pb.pts[3 * p + 1]; n_X2 = pb.pts[3 * p + 2];
    n_ptc = pb.pt_const ? (int)pb.pt_const[p] : 0;
    n_pf.template load<false>(pb.obs_cam, pb.obs_uv, pb.obs_slot, n_o0, n_o1, LPP, sl);
    if (p + nw < d.P) {
      const int pm = p + nw;
      m_o0 = pb.row_ptr[pm]; m_o1 = pb.row_ptr[pm + 1];
      m_X0 = pb.pts[3 * pm]; m_X1 = pb.pts[3 * pm + 1]; m_X2 = pb.pts[3 * pm + 2];
      m_ptc = pb.pt_const ? (int)pb.pt_const[pm] : 0;
    }
  }
  for (; p < d.P; p += nw) {
    const int o0 = n_o0, o1 = n_o1;
    const double X[3] = {n_X0, n_X1, n_X2};
    const bool pt_c = n_ptc != 0;
    const ObsPf<NPF> f_pf = n_pf;
    {
      // stage 1 -> current of the next iteration: observations of point p + nw (its bounds arrived an iteration ago)
      n_o0 = m_o0; n_o1 = m_o1; n_X0 = m_X0; n_X1 = m_X1; n_X2 = m_X2; n_ptc = m_ptc;
      if (p + nw < d.P) n_pf.template load<false>(pb.obs_cam, pb.obs_uv, pb.obs_slot, n_o0, n_o1, LPP, sl);
      // stage 2: bounds / coordinates of point p + 2 nw
      const int pm = p + 2 * nw;
      if (pm < d.P) {
        m_o0 = pb.row_ptr[pm]; m_o1 = pb.row_ptr[pm + 1];
        m_X0 = pb.pts[3 * pm]; m_X1 = pb.pts[3 * pm + 1]; m_X2 = pb.pts[3 * pm + 2];
        m_ptc = pb.pt_const ? (int)pb.pt_const[pm] : 0;
      }
    }
    double t3[3] = {0, 0, 0};
    // (the point's G and hs are requested here, in front of the Jacobian sweep, not behind it where they are used: behind
    //  the sweep every point paid their round trip -- ~1 us of ~5 -- with nothing left to overlap it)
    const double* Gp = w.G + 6 * (size_t)p;
    const double G00 = Gp[0], G01 = Gp[1], G02 = Gp[2], G11 = Gp[3], G12 = Gp[4], G22 = Gp[5];
    const double hs0 = w.hs[3 * (size_t)p], hs1 = w.hs[3 * (size_t)p + 1], hs2 = w.hs[3 * (size_t)p + 2];
    const double pd0 = w.pdamp[3 * (size_t)p], pd1 = w.pdamp[3 * (size_t)p + 1], pd2 = w.pdamp[3 * (size_t)p + 2];
    // Model cost change without a second evaluation of the Jacobians.  With m = -(F dy + E ys) the model residual of an
    // observation (Ceres: -sum m.(r + m/2)), the sum over the observations of a point is
    //   sum [F dy . r - |F dy|^2 / 2]  +  ys^T g - ys^T t3 - ys^T V ys / 2        (g = sum E^T r, t3 = sum E^T F dy, V = sum E^T E)
    // and with (V + D^2) ys = g - t3 and (V + D^2)^-1 = G G^T (point_pass):  ys^T (g - t3) = |G^-1 ys|^2 =: |z|^2, so
    //   = sum [F dy . r - |F dy|^2 / 2]  +  |z|^2 / 2  +  ys^T D^2 ys / 2.
    // The bracket is accumulated in the sweep.
    auto evaluated = [&](int pass, int o) __attribute__((always_inline)) {
      const int c = f_pf.cam(pass, pb.obs_cam, o);
      const float2 uv = f_pf.uv(pass, pb.obs_uv, o);
      const int a = d.shared ? 0 : c;
      double dyp[6], di[2] = {0.0, 0.0};
#pragma unroll
      for (int k = 0; k < 6; ++k) dyp[k] = LDSCAM ? ldy[6 * c + k] : w.dy[6 * c + k];
#pragma unroll
      for (int k = 0; k < KD; ++k) di[k] = LDSCAM ? ldi[KD * a + k] : w.dy[6 * d.C + KD * a + k];
      const double df = (KD == 2 || (KD == 1 && !d.only_k)) ? di[0] : 0.0;
      const double dk = (KD == 2) ? di[1] : ((KD == 1 && d.only_k) ? di[0] : 0.0);
      double Rg[9];
      const double* Rc = lq + 9 * c;
      if (!LDSCAM) { quat_to_R(pb.cam_q + 4 * c, Rg); Rc = Rg; }
      const ObsStep s = obs_step_R(d.model, Rc, LDSCAM ? lt + 3 * c : pb.cam_t + 3 * c, pb.intr + 4 * a, X, dyp, df, dk,
                                   (double)uv.x, (double)uv.y);
      double y[2] = {s.fy[0], s.fy[1]};
      if (d.loss != kLossTrivial) {
        const double sq = s.r[0] * s.r[0] + s.r[1] * s.r[1];
        double rho[3];
        loss_eval(d.loss, d.loss_scale, sq, rho);
        const Corrector cor(sq, rho);
#pragma unroll
        for (int rep = 0; rep < 2; ++rep) {        // fy' = C fy, then C fy' for the adjoint
          const double rty = cor.alpha_sq_norm * (s.r[0] * y[0] + s.r[1] * y[1]);
          y[0] = cor.sqrt_rho1 * (y[0] - s.r[0] * rty);
          y[1] = cor.sqrt_rho1 * (y[1] - s.r[1] * rty);
        }
      }
      double v3[3];
      s.adjoint(y, v3);
      if (!pt_c) {
#pragma unroll
        for (int k = 0; k < 3; ++k) t3[k] += Rc[k] * v3[0] + Rc[3 + k] * v3[1] + Rc[6 + k] * v3[2];
      }
    };
    for (int o = o0 + sl; o < o1; o += LPP) evaluated((o - o0) / LPP, o);
#pragma unroll
    for (int i = 0; i < 3; ++i) t3[i] = group_sum<LPP>(t3[i]);
    // ys = hs - G G^T t3
    const double u0 = G00 * t3[0], u1 = G01 * t3[0] + G11 * t3[1], u2 = G02 * t3[0] + G12 * t3[1] + G22 * t3[2];
    double ys[3];
    ys[0] = hs0 - (G00 * u0 + G01 * u1 + G02 * u2);
    ys[1] = hs1 - (G11 * u1 + G12 * u2);
    ys[2] = hs2 - (G22 * u2);
    if (sl == 0) {
      w.cand_pts[3 * (size_t)p] = X[0] - ys[0]; w.cand_pts[3 * (size_t)p + 1] = X[1] - ys[1]; w.cand_pts[3 * (size_t)p + 2] = X[2] - ys[2];
      s_step += ys[0] * ys[0] + ys[1] * ys[1] + ys[2] * ys[2];
      if (!pt_c) s_xn += X[0] * X[0] + X[1] * X[1] + X[2] * X[2];
      if (G22 != 0.0) {                                  // (constant / unobserved points: G = 0, ys = 0)
        const double z2 = ys[2] / G22, z1 = (ys[1] - G12 * z2) / G11, z0 = (ys[0] - G01 * z1 - G02 * z2) / G00;
        s_mcc += 0.5 * (z0 * z0 + z1 * z1 + z2 * z2) + 0.5 * (pd0 * ys[0] * ys[0] + pd1 * ys[1] * ys[1] + pd2 * ys[2] * ys[2]);
      }
    }
  }
  s_mcc = wave_sum(s_mcc); s_step = wave_sum(s_step); s_xn = wave_sum(s_xn);
  if (lane == 0) { red[wave][0] = s_mcc; red[wave][1] = s_step; red[wave][2] = s_xn; }
  __syncthreads();
  if (threadIdx.x < 3) w.part_F[4 * blockIdx.x + 1 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// (a launch of its own with the separate glue launches, vgg_ba_set_tile_rhs(| 4); otherwise the last workgroup of
//  cam_reduce_kernel<KD, 0> runs the body)
__global__ __launch_bounds__(256) void reduce_step_kernel(Ws w, int nparts, int C) {
  __shared__ double red[4][256];
  if (w.ctl->done) return;
  reduce_step_body<false>(w, nparts, C, red);
}

// ---------------------------------------------------------------------------------------------
void launch_point_pass(const Launch& L) {
  ProfScope ps(kProfPointPass, L.st);
  const Dims& d = L.d;
  // cameras (q, t, pose scales, constant flags: 14 doubles each) cached in LDS when they fit beside 2 workgroups/CU
  const size_t cam_lds = sizeof(double) * 19 * (size_t)d.C;
  dispatch_kd(d.kd, [&](auto kd) {
    constexpr int KD = decltype(kd)::value;
    auto launch_cy = [&](auto lpp, auto cy) {
      constexpr int LPP = decltype(lpp)::value;
      constexpr bool CY = decltype(cy)::value;
      const bool longt = long_tracks(LPP, L.d.P, L.d.O);
      // (two workgroups per CU: the compressed variant keeps 25 KB of record staging beside the camera table)
      const size_t cam_cap = (CY ? 53 : 64) * 1024;
      if (longt && LPP <= 32) {
        if (cam_lds <= cam_cap) point_pass_kernel<KD, true, CY, LPP, (LPP <= 32)><<<L.wgB, 256, cam_lds, L.st>>>(L.dp, L.w, L.opt);
        else point_pass_kernel<KD, false, CY, LPP, (LPP <= 32)><<<L.wgB, 256, 0, L.st>>>(L.dp, L.w, L.opt);
      } else if (cam_lds <= cam_cap) point_pass_kernel<KD, true, CY, LPP><<<L.wgB, 256, cam_lds, L.st>>>(L.dp, L.w, L.opt);
      else point_pass_kernel<KD, false, CY, LPP><<<L.wgB, 256, 0, L.st>>>(L.dp, L.w, L.opt);
    };
    // compressed Schur factors with 6 x 6 tile blocks (shared or constant intrinsics), full factors otherwise
    auto launch = [&](auto lpp) {
      if constexpr (KD == 0) launch_cy(lpp, std::true_type{});
      else if (d.shared) launch_cy(lpp, std::true_type{});
      else launch_cy(lpp, std::false_type{});
    };
    dispatch_lpp(L.lpp, launch);
  });
}

void launch_point_step(const Launch& L) {
  const Dims& d = L.d;
  // the camera table of point_step in LDS: R, t per camera, dy
  const size_t cam_lds = sizeof(double) * (12 * (size_t)d.C + (size_t)d.n_red);
  const bool lds_cam = cam_lds <= 64 * 1024;
  // cam_update's body in point_step's prologue: with the LDS table only (without it the sweep reads w.dy from global memory)
  const int fused = (lds_cam && !g_tuning.legacy_glue) ? 1 : 0;
  dispatch_kd(d.kd, [&](auto kd) {
    constexpr int KD = decltype(kd)::value;
    if (!fused) cam_update_kernel<KD><<<div_up(d.C + 1, 64), 64, 0, L.st>>>(L.dp, L.w);
    ProfScope ps(kProfPointStep, L.st);
    dispatch_lpp(L.lpp, [&](auto lpp) {
      constexpr int LPP = decltype(lpp)::value;
      const bool longt = long_tracks(LPP, L.d.P, L.d.O);
      if (longt && LPP <= 32) {
        if (lds_cam) point_step_kernel<KD, true, LPP, (LPP <= 32)><<<L.wgB, 256, cam_lds, L.st>>>(L.dp, L.w, fused);
        else point_step_kernel<KD, false, LPP, (LPP <= 32)><<<L.wgB, 256, 0, L.st>>>(L.dp, L.w, 0);
      } else if (lds_cam) point_step_kernel<KD, true, LPP><<<L.wgB, 256, cam_lds, L.st>>>(L.dp, L.w, fused);
      else point_step_kernel<KD, false, LPP><<<L.wgB, 256, 0, L.st>>>(L.dp, L.w, 0);
    });
  });
}

void launch_reduce_step(const Launch& L) { reduce_step_kernel<<<1, 256, 0, L.st>>>(L.w, L.wgB, L.d.C); }

}  // namespace vgg
