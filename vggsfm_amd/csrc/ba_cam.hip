// Bundle adjustment, the camera-major launches: cam_pass_kernel (the linearisation at the start point or at the candidate;
// the reduced right-hand side without tile_rhs) and cam_reduce_kernel.  The driver is ba.hip.
#include "ba_obs.hpp"

namespace vgg {

#ifndef VGG_CP_OCC_RHS
#define VGG_CP_OCC_RHS 2
#endif
#ifndef VGG_CP_OCC
#define VGG_CP_OCC 2
#endif

// ---------------------------------------------------------------------------------------------
// camera-major pass.  MODE 0: linearisation terms U_c, g_c, cost at (pb.cam_q, pb.cam_t, pb.intr, pb.pts) into w.U, w.g,
// w.costc -- the start point (vgg_ba_begin) or the candidate (phase 2, launch_linearize).  MODE 1: T_c = F^T [r - E hs | -E Ms].
template <int KD, int MODE>
__global__ __launch_bounds__(256, (MODE == 1) ? VGG_CP_OCC_RHS : VGG_CP_OCC) void cam_pass_kernel(DevProblem pb, Ws w) {
  constexpr int BD = 6 + KD;
  constexpr int NU = BD * (BD + 1) / 2;
  constexpr int NV = (MODE == 0) ? (NU + BD + 1) : (BD * (1 + KD));
  __shared__ double red[4 * NV];
  __shared__ double tot[NV];
  if (w.ctl->done) return;
  if (MODE == 1) {
    // Zero the reduced system S | rhs for the tile sums and assemble_kernel that follow (nothing touches it in between, and
    // the previous iteration is done with it): a few 16-byte stores per thread here instead of a fill launch
    zero_system_lower(w, pb.d.n_red, (int)(blockIdx.y * gridDim.x + blockIdx.x), (int)(gridDim.x * gridDim.y));
  }
  const Dims& d = pb.d;
  // grid (C, split): a camera's observations are cut into `split` contiguous slices, one workgroup each (one
  // workgroup per camera left 200 workgroups = 0.8 wavefronts per SIMD on the chip); cam_reduce_kernel adds the
  // slices in a fixed order
  const int c = blockIdx.x, split = gridDim.y;
  double q[9], t[3], in4[4];                   // q: the camera's rotation MATRIX
  quat_to_R(pb.cam_q + 4 * c, q);
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = pb.cam_t[3 * c + k];
  const int a = d.shared ? 0 : c;
#pragma unroll
  for (int k = 0; k < 4; ++k) in4[k] = pb.intr[4 * a + k];
  const unsigned camflag = pb.cam_const ? pb.cam_const[c] : 0u;
  const bool intr_c = pb.intr_const ? pb.intr_const[a] != 0 : false;
  const int kdsh = d.kdsh;
  double acc[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) acc[i] = 0.0;
  const int j_begin = pb.col_ptr[c], j_count = pb.col_ptr[c + 1] - j_begin;
  const int per = (j_count + split - 1) / split;
  const int j0 = j_begin + (int)blockIdx.y * per, j1 = min(j0 + per, j_begin + j_count);
  // Software pipeline over this thread's observations: (point index, pixel) are loaded AHEAD + 1 iterations ahead, the point
  // coordinates (and, MODE 1, its back-substitution terms) -- a gather that depends on the index -- AHEAD iterations ahead:
  // the two dependent memory round trips of an observation overlap the arithmetic of the observations before it.
  // (Without it the pass ran 5x off its instruction-issue bound at 3-4 wavefronts per SIMD; one stage less: 52 % of the
  // wave cycles still waiting.)
  constexpr int KM = (KD > 0) ? KD : 1;
  struct Gathered { double X[3], h[3], M[3 * KM]; float2 uv; int c; };   // (c: the constant-point flag as loaded, tested where it is used)
  auto gather = [&](Gathered& g, int p, float2 uv) __attribute__((always_inline)) {
    g.uv = uv;
    g.X[0] = pb.pts[3 * p]; g.X[1] = pb.pts[3 * p + 1]; g.X[2] = pb.pts[3 * p + 2];
    g.c = pb.pt_const ? (int)pb.pt_const[p] : 0;
    if (MODE == 1) {
      g.h[0] = w.hs[3 * p]; g.h[1] = w.hs[3 * p + 1]; g.h[2] = w.hs[3 * p + 2];
#pragma unroll
      for (int m = 0; m < KD; ++m)
        if (m < kdsh) {
          const double* M = w.Ms + ((size_t)p * kdsh + m) * 3;
          g.M[3 * m] = M[0]; g.M[3 * m + 1] = M[1]; g.M[3 * m + 2] = M[2];
        }
    }
  };
  // (MODE 1 carries more per observation and runs out of registers with the second gather stage: 16 bytes of scratch and
  //  0.133 -> 0.136 ms at c3, while MODE 0 goes from 0.099 to 0.087 ms -- so one stage there, two here)
  constexpr int AHEAD = (MODE == 0 && KD > 0) ? 2 : 1;     // gather stages (KD = 0, MODE 0: the second stage would cost the third wavefront per SIMD)
  Gathered g1 = {}, g2 = {};
  int j = j0 + threadIdx.x;
  int p3 = 0; float2 uv3 = make_float2(0.f, 0.f);
  if (j < j1) gather(g1, pb.cobs_pt[j], pb.cobs_uv[j]);
  if (AHEAD == 2 && j + 256 < j1) gather(g2, pb.cobs_pt[j + 256], pb.cobs_uv[j + 256]);
  if (j + 256 * AHEAD < j1) { p3 = pb.cobs_pt[j + 256 * AHEAD]; uv3 = pb.cobs_uv[j + 256 * AHEAD]; }
  for (; j < j1; j += 256) {
    const Gathered cur = g1;
    const float2 uv = cur.uv;
    const double X[3] = {cur.X[0], cur.X[1], cur.X[2]};
    const bool pt_c = cur.c != 0;
    const double h0 = cur.h[0], h1v = cur.h[1], h2 = cur.h[2];
    double Mc[3 * KM];
#pragma unroll
    for (int i = 0; i < 3 * KM; ++i) Mc[i] = cur.M[i];
    // advance the pipeline: gather for iteration j + 512 (its index arrived an iteration ago), index for j + 768
    if (AHEAD == 2) {
      g1 = g2;
      if (j + 512 < j1) gather(g2, p3, uv3);
    } else if (j + 256 < j1) gather(g1, p3, uv3);
    if (j + 256 * (AHEAD + 1) < j1) { p3 = pb.cobs_pt[j + 256 * (AHEAD + 1)]; uv3 = pb.cobs_uv[j + 256 * (AHEAD + 1)]; }
    double r[2], F[2 * BD], E[6];
    const double rho0 = eval_full<KD>(d, q, t, in4, X, uv, camflag, intr_c, pt_c, r, F, E);
    if (MODE == 0) {
      int u = 0;
#pragma unroll
      for (int i = 0; i < BD; ++i)
#pragma unroll
        for (int k = i; k < BD; ++k) acc[u++] += F[i] * F[k] + F[BD + i] * F[BD + k];
#pragma unroll
      for (int i = 0; i < BD; ++i) acc[NU + i] += F[i] * r[0] + F[BD + i] * r[1];
      acc[NU + BD] += rho0;
    } else {
      double R0[1 + KD], R1[1 + KD];
      R0[0] = r[0] - (E[0] * h0 + E[1] * h1v + E[2] * h2);
      R1[0] = r[1] - (E[3] * h0 + E[4] * h1v + E[5] * h2);
#pragma unroll
      for (int m = 0; m < KD; ++m) {
        if (m < kdsh) {
          const double* M = Mc + 3 * m;
          R0[1 + m] = -(E[0] * M[0] + E[1] * M[1] + E[2] * M[2]);
          R1[1 + m] = -(E[3] * M[0] + E[4] * M[1] + E[5] * M[2]);
        } else { R0[1 + m] = 0; R1[1 + m] = 0; }
      }
#pragma unroll
      for (int i = 0; i < BD; ++i)
#pragma unroll
        for (int m = 0; m < 1 + KD; ++m) acc[i * (1 + KD) + m] += F[i] * R0[m] + F[BD + i] * R1[m];
    }
  }
  if (MODE == 0) block_sum_scatter<NV>(acc, red, tot);
  else block_sum<NV>(acc, red, tot);
  static_assert(NV <= kCamNV, "cam_split row");
  if (threadIdx.x < NV) w.cam_split[((size_t)c * kCamSplitMax + blockIdx.y) * kCamNV + threadIdx.x] = tot[threadIdx.x];
}

// sums the `split` slices of a camera in order and stores U, g, cost (MODE 0) or T (MODE 1).
// MODE 0 runs with 256 threads (reduce_step_body's tree); step_parts > 0 (the candidate's linearisation, phase 2): the workgroup
// that arrives LAST at ctl->step_arrivals also sums reduce buffer 3 from the cameras' costs and point_step's `step_parts`
// partial sums -- it needs nothing but "every camera's cost is stored", so no launch of its own.  Nobody waits: each workgroup
// drains its stores, releases them at agent scope and takes a ticket; the one that draws C - 1 acquires and reads past its L1.
// The last arriver puts the counter back to 0 (init_kernel clears it once per solve), so an iteration that was cut short --
// ctl->done: no workgroup takes a ticket -- leaves it at 0 as well.
template <int KD, int MODE>
__global__ __launch_bounds__(MODE == 0 ? 256 : 64) void cam_reduce_kernel(DevProblem pb, Ws w, int split, int point_parts, int step_parts) {
  constexpr int BD = 6 + KD;
  constexpr int NU = BD * (BD + 1) / 2;
  constexpr int NV = (MODE == 0) ? (NU + BD + 1) : (BD * (1 + KD));
  __shared__ double red[MODE == 0 ? 4 : 1][MODE == 0 ? 256 : 1];
  if (w.ctl->done) return;
  if (MODE == 1 && blockIdx.x == 0) {            // (rides along: max of the point passes' per-workgroup gradient norms)
    double m = 0;
    for (int i = threadIdx.x; i < point_parts; i += 64) m = fmax(m, w.part_B[i]);
    m = wave_max(m);
    if (threadIdx.x == 0) w.gmax_pts[0] = m;
  }
  const Dims& d = pb.d;
  const int c = blockIdx.x, kdsh = d.kdsh;
  if (threadIdx.x < NV) {
    double tot = 0.0;
#pragma unroll 8
    for (int sp = 0; sp < split; ++sp) tot += w.cam_split[((size_t)c * kCamSplitMax + sp) * kCamNV + threadIdx.x];
    if (MODE == 0) {
      double* U = w.U + (size_t)c * BD * BD;
      if (threadIdx.x < NU) {
        int i = 0, rem = threadIdx.x;
        while (rem >= BD - i) { rem -= BD - i; ++i; }
        const int k = i + rem;
        U[i * BD + k] = tot;
        U[k * BD + i] = tot;
      } else if (threadIdx.x < NU + BD) {
        w.g[(size_t)c * BD + threadIdx.x - NU] = tot;
      } else {
        w.costc[c] = tot;
      }
    } else {
      // stored with row stride (1 + kdsh)
      const int i = threadIdx.x / (1 + KD), m = threadIdx.x - i * (1 + KD);
      if (m < 1 + kdsh) w.T[((size_t)c * BD + i) * (1 + kdsh) + m] = tot;
    }
  }
  if constexpr (MODE == 0) {
    if (step_parts <= 0) return;                   // (uniform: the start linearisation, or the separate reduce_step launch)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // every storing wavefront drains its stores
    __syncthreads();
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const int ticket = __hip_atomic_fetch_add(&w.ctl->step_arrivals, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
      const bool last = ticket == (int)gridDim.x - 1;
      if (last) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      red[0][0] = last ? 1.0 : 0.0;
    }
    __syncthreads();
    const bool last = red[0][0] != 0.0;
    __syncthreads();                               // (red is reused by the sums)
    if (!last) return;
    reduce_step_body<true>(w, step_parts, d.C, red);
    if (threadIdx.x == 0) {
      w.ctl->merged_step_sums += 1;
      __hip_atomic_store(&w.ctl->step_arrivals, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// U_c, g_c, cost of the local observations at the parameters `dp` points to, into the buffer `w` points to: the start point
// into reduce buffer 0 (vgg_ba_begin), the candidate into lin_cand (phase 2).  One kernel pair for both, so that the
// linearisation an accepted candidate leaves behind is bit for bit the one a pass at the new x would compute.
void launch_linearize(const Launch& L, const DevProblem& dp, const Ws& w, int step_parts) {
  // step_parts > 0: the last workgroup of cam_reduce also sums reduce buffer 3 (the candidate of phase 2)
  const int split = cam_split_for(L.d.C, L.d.O);
  dispatch_kd(L.d.kd, [&](auto kd) {
    constexpr int KD = decltype(kd)::value;
    cam_pass_kernel<KD, 0><<<dim3(L.d.C, split), 256, 0, L.st>>>(dp, w);
    cam_reduce_kernel<KD, 0><<<L.d.C, 256, 0, L.st>>>(dp, w, split, 0, step_parts);
  });
}

// T_c = F^T [r - E hs | -E Ms] per camera (without tile_rhs); the pass also zeroes the reduced system: no fill launch
void launch_cam_rhs(const Launch& L) {
  ProfScope ps(kProfCamRhs, L.st);
  const int split = cam_split_for(L.d.C, L.d.O);
  dispatch_kd(L.d.kd, [&](auto kd) {
    constexpr int KD = decltype(kd)::value;
    cam_pass_kernel<KD, 1><<<dim3(L.d.C, split), 256, 0, L.st>>>(L.dp, L.w);
    cam_reduce_kernel<KD, 1><<<L.d.C, 64, 0, L.st>>>(L.dp, L.w, split, L.wgB, 0);
  });
}

}  // namespace vgg
