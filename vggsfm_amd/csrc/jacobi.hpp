// The small symmetric eigen-solvers of the geometry kernels, all cyclic Jacobi: one row per lane for the 9x9 matrices
// (fundamental.hip, essential.hip; the 12x12 of epnp.hip keeps the loop written out, it was measured slower through the
// helper, and takes the selection by rank), in one thread's registers for the 3x3 (fundamental.hip, sim3.hip, and the
// one-sided SVD of kabsch3.hpp through jacobi_cs) and the 4x4 (triangulate.hip, multiview.hip).
// Floating-point contraction is set per translation unit (Makefile), and a template in a header is compiled under the
// setting of the file that includes it: sharing the source here does not share the rounding.  triangulate.hip runs
// smallest_eigvec4 contracted, every other file runs what it takes from here unfused.
// The 3x3 and the 4x4 forms stay apart: they rotate by different formulas (jacobi_cs against the 1e-300 guard with an early
// exit), and one body would change the bits of one of them.
#pragma once
#include "common.hpp"

namespace vgg {

// the rotation (c, s) that zeroes a_pq; the identity where it is zero already
__device__ inline void jacobi_cs(double app, double aqq, double apq, double& c, double& s) {
  const bool rot = apq != 0.0;
  const double tau = (aqq - app) / (2.0 * (rot ? apq : 1.0));
  const double t = ((tau >= 0.0) ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
  const double cc = 1.0 / sqrt(1.0 + t * t);
  c = rot ? cc : 1.0;
  s = rot ? t * cc : 0.0;
}

// kSweeps sweeps over a symmetric N x N matrix held one row per lane: lane g < N of a group of kWidth lanes passes row g of
// the matrix in a and of the start of V (the identity) in v, and gets row g of the rotated matrix (eigenvalue j = a[j] of
// lane j) and of V (columns = eigenvectors) back.  Lanes g >= N pass any row; what they get back means nothing.
// (The sweeps run on copies: a helper that works through its pointer arguments is optimised before it is inlined, and the
//  conditional row update then stays as branches instead of selects.)
template <int N, int kWidth, int kSweeps>
__device__ __forceinline__ void jacobi_rows(double* a_io, double* v_io, int g) {
  double a[N], v[N];
#pragma unroll
  for (int j = 0; j < N; ++j) { a[j] = a_io[j]; v[j] = v_io[j]; }
  for (int sw = 0; sw < kSweeps; ++sw) {
#pragma unroll
    for (int p = 0; p < N - 1; ++p) {
#pragma unroll
      for (int q = p + 1; q < N; ++q) {
        const double app = __shfl(a[p], p, kWidth), aqq = __shfl(a[q], q, kWidth), apq = __shfl(a[q], p, kWidth);
        double c, s;
        jacobi_cs(app, aqq, apq, c, s);
        { const double cp = a[p], cq = a[q]; a[p] = c * cp - s * cq; a[q] = s * cp + c * cq; }      // columns p, q
        double rp[N], rq[N];
#pragma unroll
        for (int j = 0; j < N; ++j) { rp[j] = __shfl(a[j], p, kWidth); rq[j] = __shfl(a[j], q, kWidth); }
        if (g == p) {
#pragma unroll
          for (int j = 0; j < N; ++j) a[j] = c * rp[j] - s * rq[j];
        } else if (g == q) {
#pragma unroll
          for (int j = 0; j < N; ++j) a[j] = s * rp[j] + c * rq[j];
        }
        { const double vp = v[p], vq = v[q]; v[p] = c * vp - s * vq; v[q] = s * vp + c * vq; }      // V columns
      }
    }
  }
#pragma unroll
  for (int j = 0; j < N; ++j) { a_io[j] = a[j]; v_io[j] = v[j]; }
}

// After jacobi_rows: this lane's component of the eigenvectors of the K smallest eigenvalues (ties: the lower index first).
// nb[k] belongs to the k-th smallest, or, with kSmallestLast, nb[K - 1 - k] does.
template <int N, int K, int kWidth, bool kSmallestLast>
__device__ __forceinline__ void smallest_by_rank(const double* a, const double* v, double* nb) {
  double ev[N];
#pragma unroll
  for (int j = 0; j < N; ++j) ev[j] = __shfl(a[j], j, kWidth);
#pragma unroll
  for (int k = 0; k < K; ++k) nb[k] = 0.0;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    int rank = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) rank += (ev[i] < ev[j] || (ev[i] == ev[j] && i < j)) ? 1 : 0;
#pragma unroll
    for (int k = 0; k < K; ++k) nb[k] = (rank == (kSmallestLast ? K - 1 - k : k)) ? v[j] : nb[k];
  }
}

// kSweeps sweeps over a symmetric 3x3 in registers: A ends (nearly) diagonal; with kVectors, V (the identity on entry)
// collects the rotations: its columns are the eigenvectors; without, V is not touched.  (On copies, as jacobi_rows: the
// callers' assembly is then what their own loops gave.)
template <int kSweeps, bool kVectors>
__device__ __forceinline__ void jacobi_sym3(double (*A_io)[3], double (*V_io)[3]) {
  double A[3][3], V[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) { A[i][j] = A_io[i][j]; V[i][j] = kVectors ? V_io[i][j] : 0.0; }
  for (int sw = 0; sw < kSweeps; ++sw) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        double c, s;
        jacobi_cs(A[p][p], A[q][q], A[p][q], c, s);
#pragma unroll
        for (int i = 0; i < 3; ++i) { const double cp = A[i][p], cq = A[i][q]; A[i][p] = c * cp - s * cq; A[i][q] = s * cp + c * cq; }
#pragma unroll
        for (int j = 0; j < 3; ++j) { const double rp = A[p][j], rq = A[q][j]; A[p][j] = c * rp - s * rq; A[q][j] = s * rp + c * rq; }
        if (kVectors) {
#pragma unroll
          for (int i = 0; i < 3; ++i) { const double vp = V[i][p], vq = V[i][q]; V[i][p] = c * vp - s * vq; V[i][q] = s * vp + c * vq; }
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) { A_io[i][j] = A[i][j]; if (kVectors) V_io[i][j] = V[i][j]; }
}

// eigenvector of the smallest eigenvalue (first minimum) of the symmetric 4x4 (a: 00 01 02 03 11 12 13 22 23 33), in
// registers: at most kSweeps sweeps, done once the off-diagonal sum is at or below tol times the diagonal's
template <int kSweeps>
__device__ __forceinline__ void smallest_eigvec4(const double* a, double tol, double* v) {
  double A[4][4] = {{a[0], a[1], a[2], a[3]}, {a[1], a[4], a[5], a[6]}, {a[2], a[5], a[7], a[8]}, {a[3], a[6], a[8], a[9]}};
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
#pragma unroll 1
  for (int sweep = 0; sweep < kSweeps; ++sweep) {
    double off = 0.0, dsum = 0.0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      dsum += fabs(A[p][p]);
#pragma unroll
      for (int q = p + 1; q < 4; ++q) off += fabs(A[p][q]);
    }
    if (!(off > 1e-300) || off <= tol * dsum) break;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[p][q];
        if (fabs(apq) > 1e-300) {
          const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
          const double t = ((theta >= 0.0) ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const double akp = A[k][p], akq = A[k][q];
            A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const double apk = A[p][k], aqk = A[q][k];
            A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const double vkp = V[k][p], vkq = V[k][q];
            V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
          }
        }
      }
    }
  }
  int best = 0;
  double bv = A[0][0];
#pragma unroll
  for (int k = 1; k < 4; ++k) if (A[k][k] < bv) { bv = A[k][k]; best = k; }
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = (best == 0) ? V[k][0] : (best == 1) ? V[k][1] : (best == 2) ? V[k][2] : V[k][3];
}

}  // namespace vgg
