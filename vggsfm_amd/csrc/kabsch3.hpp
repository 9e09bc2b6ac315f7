// The 3x3 Procrustes step shared by the EPnP solver (epnp.hip) and the Sim(3) alignment (sim3.hip).  Compiled without
// floating-point contraction in both files.
#pragma once
#include "common.hpp"
#include "jacobi.hpp"

namespace vgg {

constexpr int kSweeps3 = 10;         // one-sided Jacobi sweeps of the 3x3 covariance

// Umeyama with scale from the covariance C (row = world axis, column = camera axis): C = U S V^T by one-sided Jacobi
// (C V = U S), R = U diag(1, 1, det(U V^T)) V^T, returns trace(diag(1, 1, det) S).  With u3' = u1 x u2 the third term of R
// is det(V) u3' v3^T and its singular value enters as det(V) (c3 . u3'): the smallest singular value is never divided by
__device__ __forceinline__ double kabsch3(const double* C, double* R) {
  double a[3][3], v[3][3];             // a[i] = column i of C V, v[i] = column i of V
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int c = 0; c < 3; ++c) { a[i][c] = C[3 * c + i]; v[i][c] = (i == c) ? 1.0 : 0.0; }
  for (int sw = 0; sw < kSweeps3; ++sw) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        const double app = (a[p][0] * a[p][0] + a[p][1] * a[p][1]) + a[p][2] * a[p][2];
        const double aqq = (a[q][0] * a[q][0] + a[q][1] * a[q][1]) + a[q][2] * a[q][2];
        const double apq = (a[p][0] * a[q][0] + a[p][1] * a[q][1]) + a[p][2] * a[q][2];
        double c, s;
        jacobi_cs(app, aqq, apq, c, s);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double ap = a[p][k], aq = a[q][k], vp = v[p][k], vq = v[q][k];
          a[p][k] = c * ap - s * aq; a[q][k] = s * ap + c * aq;
          v[p][k] = c * vp - s * vq; v[q][k] = s * vp + c * vq;
        }
      }
    }
  }
  double n2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) n2[i] = (a[i][0] * a[i][0] + a[i][1] * a[i][1]) + a[i][2] * a[i][2];
  // descending order of the column norms (ties: the lower index first)
  int ord[3] = {0, 0, 0};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    int rank = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) rank += (n2[j] > n2[i] || (n2[j] == n2[i] && j < i)) ? 1 : 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) ord[k] = (rank == k) ? i : ord[k];
  }
  double as[3][3], vs[3][3], sg[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    sg[k] = sqrt(ord[k] == 0 ? n2[0] : (ord[k] == 1 ? n2[1] : n2[2]));
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      as[k][c] = ord[k] == 0 ? a[0][c] : (ord[k] == 1 ? a[1][c] : a[2][c]);
      vs[k][c] = ord[k] == 0 ? v[0][c] : (ord[k] == 1 ? v[1][c] : v[2][c]);
    }
  }
  double u1[3], u2[3], u3[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) { u1[c] = as[0][c] / sg[0]; u2[c] = as[1][c] / sg[1]; }
  u3[0] = u1[1] * u2[2] - u1[2] * u2[1]; u3[1] = u1[2] * u2[0] - u1[0] * u2[2]; u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
  const double dv = (vs[0][0] * (vs[1][1] * vs[2][2] - vs[1][2] * vs[2][1]) - vs[0][1] * (vs[1][0] * vs[2][2] - vs[1][2] * vs[2][0])) +
                    vs[0][2] * (vs[1][0] * vs[2][1] - vs[1][1] * vs[2][0]);
  const double sd = (dv >= 0.0) ? 1.0 : -1.0;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) R[3 * r + c] = (u1[r] * vs[0][c] + u2[r] * vs[1][c]) + sd * (u3[r] * vs[2][c]);
  const double s3 = (as[2][0] * u3[0] + as[2][1] * u3[1]) + as[2][2] * u3[2];
  return (sg[0] + sg[1]) + sd * s3;
}

}  // namespace vgg
