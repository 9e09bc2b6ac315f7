// Device code shared by the two-view estimators (fundamental.hip, essential.hip): the 3x3 product, the squared Sampson
// distance, the scoring kernel, the selected-hypothesis load and the 9x9 Gram accumulation and reduction (the matrix's
// eigen-solve is jacobi.hpp's, the fixed-order block reduction common.hpp's).  Compiled without floating-point contraction in both files.  Entries: vgg_fmat_score
// and vgge_emat_score stay apart and launch the one two_view_score_kernel; vgg_fmat_residuals (fundamental.hip) is shared
// as it is -- it gives the residuals of either flow's winner.
#pragma once
#include "common.hpp"

namespace vgg {

constexpr double kBig = 1e6;         // residual of an invalid match
constexpr int kSweeps9 = 10;         // cyclic Jacobi sweeps of a 9x9 matrix (fmat8_kernel, five_point_from_gram)
constexpr int kHypPerWave = 4;       // hypotheses scored per sweep of a wavefront: the points are read once for all of them

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

// ------------------------------------------------------------------------------------------------ scoring
// Four wavefronts per workgroup, kHyp hypotheses (3x3, p2^T M p1 = 0) of pair blockIdx.y per wavefront: squared Sampson
// distance of all N matches in one sweep (coalesced, the pair's points stay in L2 for its K hypotheses), inlier count and
// residual sum; -1 and 0.0 for a dead hypothesis.  vmask null: every match usable.  thr null: thr_all for every pair.
template <int kHyp>
__global__ __launch_bounds__(256) void two_view_score_kernel(const double* __restrict__ pts1, const double* __restrict__ pts2,
                                                            const uint8_t* __restrict__ vmask, const double* __restrict__ Mall,
                                                            const uint8_t* __restrict__ mvalid, const double* __restrict__ thr,
                                                            double thr_all, int B, int N, int K, int32_t* __restrict__ counts,
                                                            double* __restrict__ rsums) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long k0 = ((long)blockIdx.x * 4 + wave) * kHyp;
  const int b = blockIdx.y;
  if (k0 >= K) return;
  const double thr_sq = thr ? thr[b] : thr_all;
  double M[kHyp][9];
  bool live[kHyp];
  bool any = false;
#pragma unroll
  for (int h = 0; h < kHyp; ++h) {
    const long k = k0 + h;
    live[h] = k < K && mvalid[(size_t)b * K + (k < K ? k : 0)];
    any = any || live[h];
#pragma unroll
    for (int i = 0; i < 9; ++i) M[h][i] = live[h] ? Mall[((size_t)b * K + k) * 9 + i] : 0.0;
  }
  const double* p1 = pts1 + (size_t)b * N * 2;
  const double* p2 = pts2 + (size_t)b * N * 2;
  const uint8_t* vm = vmask ? vmask + (size_t)b * N : nullptr;
  int c[kHyp];
  double s[kHyp];
#pragma unroll
  for (int h = 0; h < kHyp; ++h) { c[h] = 0; s[h] = 0.0; }
  if (any) {
    for (int n = lane; n < N; n += 64) {
      const double u1 = p1[2 * n], v1 = p1[2 * n + 1], u2 = p2[2 * n], v2 = p2[2 * n + 1];
      const bool usable = !vm || vm[n];
#pragma unroll
      for (int h = 0; h < kHyp; ++h) {
        const double r = sampson_sq(M[h], u1, v1, u2, v2);
        const bool in = r <= thr_sq && usable;
        c[h] += in ? 1 : 0;
        s[h] = s[h] + (in ? r : 0.0);
      }
    }
  }
#pragma unroll
  for (int h = 0; h < kHyp; ++h) {
    const int ch = wave_sum_i(c[h]);
    const double sh = wave_sum(s[h]);
    if (lane == 0 && k0 + h < K) {
      counts[(size_t)b * K + k0 + h] = live[h] ? ch : -1;
      rsums[(size_t)b * K + k0 + h] = live[h] ? sh : 0.0;
    }
  }
}

// ------------------------------------------------------------------------------------------------ local optimisation
// M = hypothesis sel[b][l] of src (B, Ksrc, 9); zeros and false where the index is out of range or the hypothesis is dead
__device__ inline bool load_selected(const double* __restrict__ src, const int32_t* __restrict__ src_counts,
                                     const int32_t* __restrict__ sel, int b, int l, int Ksrc, int L, double* M) {
  const int k = sel[(size_t)b * L + l];
  const bool ok = k >= 0 && k < Ksrc && src_counts[(size_t)b * Ksrc + (k >= 0 && k < Ksrc ? k : 0)] >= 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) M[i] = ok ? src[((size_t)b * Ksrc + k) * 9 + i] : 0.0;
  return ok;
}

// acc (the 45 entries of the upper triangle, row by row) += (m r)(m r)^T for a 9-row r and its mask or weight m
__device__ __forceinline__ void gram_add(double* acc, const double* r, double m) {
  double row[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) row[i] = r[i] * m;
  int e = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i)
#pragma unroll
    for (int j = i; j < 9; ++j) { acc[e] = acc[e] + row[i] * row[j]; ++e; }
}

// Ms (symmetric) = the sum of acc over the 256 threads: nine passes of block_tree_sum<9>, pass i with row i of the triangle
// in slots i..8.  Slot 0 of the last pass is free and carries `extra`; its sum is returned (to every thread)
__device__ inline double gram_reduce(double (*red)[256], const double* acc, double (*Ms)[9], double extra = 0.0) {
  double total = 0.0;
  int e = 0;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    double vals[9], outs[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) vals[j] = (j >= i) ? acc[e + (j - i)] : ((i == 8 && j == 0) ? extra : 0.0);
    block_tree_sum<9>(red, vals, outs);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int j = 0; j < 9; ++j)
        if (j >= i) { Ms[i][j] = outs[j]; Ms[j][i] = outs[j]; }
    }
    if (i == 8) total = outs[0];
    e += 9 - i;
  }
  return total;
}

}  // namespace vgg
