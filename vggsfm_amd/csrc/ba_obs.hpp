// Bundle adjustment: the __device__ helpers that kernels of more than one unit share -- the per-observation residual and
// Jacobians and the block sums (camera and point passes), zero_system_lower (cam_pass<RHS>, point_pass), reduce_step_body
// (cam_reduce's last arriver, reduce_step_kernel).
#pragma once
#include "ba_types.hpp"

namespace vgg {

// ---------------------------------------------------------------------------------------------
// One observation: corrected residual and corrected, constant-masked, UNSCALED Jacobians.
//   F[2][6+KD]  (pose tangent 6, refined intrinsics KD), E[2][3] (point); Rm = rotation matrix of the camera (row-major)
// (camera, pixel, slot) of the first N observations of a lane, prefetched with the point.  Named scalar members and
// explicit selects: arrays filled in (later unrolled) loops stayed dynamically indexed stack objects -- scratch.
template <int N>
struct ObsPf {
  static_assert(N == 2 || N == 4, "prefetch depth");
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0, s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  float2 u0 = make_float2(0.f, 0.f), u1 = make_float2(0.f, 0.f), u2 = make_float2(0.f, 0.f), u3 = make_float2(0.f, 0.f);
  template <bool SLOT>
  __device__ __forceinline__ void load(const int32_t* cam, const float2* uv, const int32_t* slot, int o0, int o1, int stride, int sl) {
    int o = o0 + sl;
    if (o < o1) { c0 = cam[o]; u0 = uv[o]; if (SLOT) s0 = slot[o]; }
    o += stride;
    if (o < o1) { c1 = cam[o]; u1 = uv[o]; if (SLOT) s1 = slot[o]; }
    if (N == 4) {
      o += stride;
      if (o < o1) { c2 = cam[o]; u2 = uv[o]; if (SLOT) s2 = slot[o]; }
      o += stride;
      if (o < o1) { c3 = cam[o]; u3 = uv[o]; if (SLOT) s3 = slot[o]; }
    }
  }
  template <typename T>
  __device__ __forceinline__ static T pick(T a0, T a1, T a2, T a3, int k) {
    const T lo = (k & 1) ? a1 : a0, hi = (k & 1) ? a3 : a2;
    return (N == 4 && (k & 2)) ? hi : lo;
  }
  __device__ __forceinline__ int cam(int k, const int32_t* src, int o) const { return k < N ? pick(c0, c1, c2, c3, k) : src[o]; }
  __device__ __forceinline__ int slot(int k, const int32_t* src, int o) const { return k < N ? pick(s0, s1, s2, s3, k) : src[o]; }
  __device__ __forceinline__ float2 uv(int k, const float2* src, int o) const {
    if (k >= N) return src[o];
    return make_float2(pick(u0.x, u1.x, u2.x, u3.x, k), pick(u0.y, u1.y, u2.y, u3.y, k));
  }
};

struct CamR {                                    // rotation matrix of a quaternion in global memory (paths without the LDS cache)
  double R[9];
  __device__ __forceinline__ explicit CamR(const double* q) { quat_to_R(q, R); }
};

template <int KD>
__device__ __forceinline__ double eval_full(const Dims& d, const double* Rm, const double* t, const double* in4,
                                            const double* X, float2 uv, unsigned camflag, bool intr_c, bool pt_c,
                                            double* r, double* F, double* E, double* Jw = nullptr) {
  constexpr int BD = 6 + KD;
  double Jp[12], Ji[4];
  obs_eval_R(d.model, Rm, t, in4, X, (double)uv.x, (double)uv.y, r, Jp, Ji, E);
#pragma unroll
  for (int row = 0; row < 2; ++row) {
#pragma unroll
    for (int k = 0; k < 6; ++k) F[row * BD + k] = Jp[row * 6 + k];
    if (KD == 2) { F[row * BD + 6] = Ji[row * 2]; F[row * BD + 7] = Ji[row * 2 + 1]; }
    if (KD == 1) F[row * BD + 6] = d.only_k ? Ji[row * 2 + 1] : Ji[row * 2];
  }
  const double s = r[0] * r[0] + r[1] * r[1];
  double rho[3];
  loss_eval(d.loss, d.loss_scale, s, rho);
  if (d.loss != kLossTrivial) {
    Corrector c(s, rho);
    c.jac<BD>(r, F);
    c.jac<3>(r, E);
    r[0] *= c.residual_scaling; r[1] *= c.residual_scaling;
  }
  // Jw = corrected d r / d (R X + t) (2 x 3) BEFORE the constant-parameter masks: the translation columns of F
  if (Jw) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { Jw[k] = F[3 + k]; Jw[3 + k] = F[BD + 3 + k]; }
  }
  if (camflag) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (camflag & 1u) { F[k] = 0; F[BD + k] = 0; }
      if ((camflag & 1u) || (camflag & (2u << k))) { F[3 + k] = 0; F[BD + 3 + k] = 0; }
    }
  }
  if (intr_c) {
#pragma unroll
    for (int k = 0; k < KD; ++k) { F[6 + k] = 0; F[BD + 6 + k] = 0; }
  }
  if (pt_c) {
#pragma unroll
    for (int k = 0; k < 6; ++k) E[k] = 0;
  }
  return rho[0];
}

__device__ __forceinline__ double loss_rho0(const Dims& d, double s) {
  double rho[3];
  loss_eval(d.loss, d.loss_scale, s, rho);
  return rho[0];
}

// block-wide sum of NV per-thread values (256 threads); result valid on thread 0..NV-1 via out[]
template <int NV>
__device__ __forceinline__ void block_sum(double* v, double* lds /* [4][NV] */, double* out /* lds [NV] */) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const double s = wave_sum(v[i]);
    if (lane == 0) lds[wave * NV + i] = s;
  }
  __syncthreads();
  if (threadIdx.x < NV) out[threadIdx.x] = lds[threadIdx.x] + lds[NV + threadIdx.x] + lds[2 * NV + threadIdx.x] + lds[3 * NV + threadIdx.x];
  __syncthreads();
}

// block_sum with the wave sums as a reduce-scatter butterfly (crosslane.hpp, wave_reduce_scatter): the same bits, value i of a
// wavefront ends in ONE lane instead of in all
template <int NV>
__device__ __forceinline__ void block_sum_scatter(double* v, double* lds /* [4][NV] */, double* out /* lds [NV] */) {
  static_assert(NV <= 64, "one value per lane at the end");
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  wave_reduce_scatter<NV, 32>(v, lane, NV, 0, lds + wave * NV);
  __syncthreads();
  if (threadIdx.x < NV) out[threadIdx.x] = lds[threadIdx.x] + lds[NV + threadIdx.x] + lds[2 * NV + threadIdx.x] + lds[3 * NV + threadIdx.x];
  __syncthreads();
}

// Zeroes the part of the reduced system S | rhs that anything reads: only the lower triangle is ever filled (tile_reduce_kernel
// and assemble_kernel write S[hi][lo], the factorisation and pack_lower_kernel read it), so row i is cleared up to the end of
// the 64-column block of its diagonal element and the upper triangle is left alone -- half the stores of a full clear (at the
// 6002 x 6002 system of the final joint adjustment of configs[4]: 144 of 288 MB per iteration; vgg_ba_begin clears the whole
// S | rhs once, so with the phase API the upper triangle stays zero).  Workgroup `wg` of `nwg` takes the rows wg, wg + nwg, ...;
// row n is the right-hand side.
__device__ __forceinline__ void zero_system_lower(const Ws& w, int n, int wg, int nwg) {
  const bool even = (n & 1) == 0;                 // (rows 16-byte aligned)
  for (int row = wg; row <= n; row += nwg) {
    const int len = (row < n) ? min(n, 64 * (row / 64 + 1)) : n;
    double* dst = w.sys + (size_t)row * n;
    if (even) {
      double2* d2 = reinterpret_cast<double2*>(dst);
      for (int c = threadIdx.x; c < (len + 1) / 2; c += 256) d2[c] = make_double2(0.0, 0.0);
    } else {
      for (int c = threadIdx.x; c < len; c += 256) dst[c] = 0.0;
    }
  }
}

// reduce buffer 3: [0] the candidate's cost (sum over the cameras of cam_pass<CAND>'s sums), [1..3] the point_step sums.
// 256 threads; BYPASS: the partial sums were stored by other workgroups of the SAME launch (cam_reduce_kernel's last arriver)
// and are loaded past this CU's L1.
template <bool BYPASS>
__device__ __forceinline__ void reduce_step_body(const Ws& w, int nparts, int C, double (*red)[256]) {
  auto ld = [](const double* p) -> double {
    return BYPASS ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p;
  };
  double s[4] = {0, 0, 0, 0};
  for (int i = threadIdx.x; i < C; i += 256) s[0] += ld(w.cost_cand + i);
  for (int i = threadIdx.x; i < nparts; i += 256)
    for (int k = 1; k < 4; ++k) s[k] += ld(w.part_F + 4 * i + k);
  for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = s[k];
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (threadIdx.x < st) for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + st];
    __syncthreads();
  }
  if (threadIdx.x < 4) w.stepsum[threadIdx.x] = red[threadIdx.x][0];
}

}  // namespace vgg
