// Device helpers shared by the two-view estimators (fundamental.hip, essential.hip): the 3x3 product, the squared Sampson
// distance, the Jacobi rotation and the fixed-order block reduction.  Compiled without floating-point contraction in both files.
#pragma once
#include "common.hpp"

namespace vgg {

constexpr double kBig = 1e6;         // residual of an invalid match

__device__ inline void jacobi_cs(double app, double aqq, double apq, double& c, double& s) {
  const bool rot = apq != 0.0;
  const double tau = (aqq - app) / (2.0 * (rot ? apq : 1.0));
  const double t = ((tau >= 0.0) ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
  const double cc = 1.0 / sqrt(1.0 + t * t);
  c = rot ? cc : 1.0;
  s = rot ? t * cc : 0.0;
}

// C = A B (3x3 row-major), terms added left to right
__device__ __forceinline__ void mat3_ab(const double* A, const double* B, double* C) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

// squared Sampson distance of (u1,v1) <-> (u2,v2) under p2^T F p1 = 0
__device__ inline double sampson_sq(const double* __restrict__ F, double u1, double v1, double u2, double v2) {
  const double l0 = (F[0] * u1 + F[1] * v1) + F[2];
  const double l1 = (F[3] * u1 + F[4] * v1) + F[5];
  const double l2 = (F[6] * u1 + F[7] * v1) + F[8];
  const double m0 = (F[0] * u2 + F[3] * v2) + F[6];
  const double m1 = (F[1] * u2 + F[4] * v2) + F[7];
  const double num = (u2 * l0 + v2 * l1) + l2;
  const double den = (l0 * l0 + l1 * l1) + (m0 * m0 + m1 * m1);
  const double r = (num * num) / den;
  return isfinite(r) ? r : kBig;
}

// fixed-order reduction of Q quantities over the 256 threads: halving tree (t, t + 128), (t, t + 64), ...
template <int Q>
__device__ inline void block_tree_sum(double (*red)[256], const double* val, double* out) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int q = 0; q < Q; ++q) red[q][tid] = val[q];
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) {
#pragma unroll
      for (int q = 0; q < Q; ++q) red[q][tid] = red[q][tid] + red[q][tid + st];
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) out[q] = red[q][0];
  __syncthreads();
}

}  // namespace vgg
