// EPnP (vggsfm/two_view_geo/perspective_n_points.py:36-437, efficient_pnp) and the local optimisation of the P3P RANSAC
// of p3p.hip by it.  DESIGN.md section 17.
//
// float64, no FMA contraction (-ffp-contract=off), no transcendental functions, no atomics, every sum in a fixed order.
// One workgroup of 256 threads per problem; epnp_block() is the solver both uses share:
//   1  centroid of the weighted points (block tree).  The control points are the centroid plus the three unit axes and
//      the centroid itself, so the barycentric coordinates are  a = (x - mean, 1 - sum)  in closed form
//   2  M^T M = sum_n (a a^T) (x) G(u, v) with G = [1 0 -u; 0 1 -v; -u -v u^2+v^2]: its 78 distinct entries are the 40 sums
//      of a_j a_k {1, u, v, u^2 + v^2}; with the four sums of a_j that is 4 block trees of 11 quantities
//   3  first wavefront: cyclic Jacobi on the 12x12 matrix, one row per lane, width-16 shuffles (as five_point_from_gram);
//      the eigenvectors of the four smallest eigenvalues in ascending order, each with its largest component positive
//   4  thread k < 4 is candidate k: 0 = the kernel vector alone, 1..3 = the least-squares solves (Householder QR) on the
//      column subsets [0,4,5,6], [0,4,1], [0,4,1,5,7] of the 6x10 matrix of _kernel_vec_distances; then its sign (weighted
//      mean depth), and Umeyama with scale.  x_cam is linear in a, so every sum of the alignment is a combination of the
//      sums of pass 2: no sweep over the points.  The 3x3 SVD is a one-sided Jacobi
//   5  err_2d and err_3d of the candidates in one sweep (block tree of 8); the winner is the first minimum of err_2d
// A masked-out point is skipped: nothing read from its slots enters a sum.
#include "common.hpp"
#include "jacobi.hpp"
#include "kabsch3.hpp"
#include "support.hpp"
#include "../../include/vggsfm_amd_pnp.h"

namespace vgg {

constexpr int kSweeps12 = 12;        // Jacobi sweeps of the 12x12 matrix
constexpr int kLoMinInliers = 6;     // the smallest set the local optimisation hands to EPnP
constexpr double kEps = 1e-9;        // the reference's clamps

struct EpnpShared {
  double red[11][256];
  double sums[44];     // [10 g + p]: sum of a_j a_k {1, u, v, u^2 + v^2}[g], p = pair(j <= k); [40 + j]: sum of a_j
  double G[12][12];
  double kern[4][12];  // eigenvector k (ascending eigenvalue), component 3 j + c = coordinate c of control point j
  double cc[4][12];    // control points of candidate k in camera coordinates, sign fixed, not yet divided by the scale
  double R[4][9], T[4][3], sc[4];
  double Lm[6][10], rhs[6];
};

__host__ __device__ constexpr int pair4(int j, int k) {      // j <= k
  return (j == 0 ? 0 : (j == 1 ? 4 : (j == 2 ? 7 : 9))) + (k - j);
}
__device__ __forceinline__ int pair4_any(int j, int k) { return j <= k ? pair4(j, k) : pair4(k, j); }
__device__ __forceinline__ double shfl16(double v, int src) { return __shfl(v, src, 16); }

__device__ __forceinline__ void alphas_of(const double* x, size_t n, const double* mean, double* a) {
  a[0] = x[3 * n] - mean[0]; a[1] = x[3 * n + 1] - mean[1]; a[2] = x[3 * n + 2] - mean[2];
  a[3] = 1.0 - ((a[0] + a[1]) + a[2]);
}

// least squares of a 6 x K system by Householder QR; A and b are overwritten.  A rank-deficient system divides by zero:
// the candidate is then not finite and the problem is flagged
template <int K>
__device__ __forceinline__ void lstsq6(double (*A)[K], double* b, double* beta) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double t2 = 0.0;
#pragma unroll
    for (int i = k + 1; i < 6; ++i) t2 = t2 + A[i][k] * A[i][k];
    const double nrm = sqrt(A[k][k] * A[k][k] + t2);
    const double alpha = (A[k][k] >= 0.0) ? -nrm : nrm;
    const double v0 = A[k][k] - alpha;
    const double vn2 = v0 * v0 + t2;
#pragma unroll
    for (int j = k + 1; j < K; ++j) {
      double dot = v0 * A[k][j];
#pragma unroll
      for (int i = k + 1; i < 6; ++i) dot = dot + A[i][k] * A[i][j];
      const double f = 2.0 * dot / vn2;
      A[k][j] = A[k][j] - f * v0;
#pragma unroll
      for (int i = k + 1; i < 6; ++i) A[i][j] = A[i][j] - f * A[i][k];
    }
    {
      double dot = v0 * b[k];
#pragma unroll
      for (int i = k + 1; i < 6; ++i) dot = dot + A[i][k] * b[i];
      const double f = 2.0 * dot / vn2;
      b[k] = b[k] - f * v0;
#pragma unroll
      for (int i = k + 1; i < 6; ++i) b[i] = b[i] - f * A[i][k];
    }
    A[k][k] = alpha;
  }
#pragma unroll
  for (int k = K - 1; k >= 0; --k) {
    double s = b[k];
#pragma unroll
    for (int j = k + 1; j < K; ++j) s = s - A[k][j] * beta[j];
    beta[k] = s / A[k][k];
  }
}

// entry t < 60 of the 6 x 10 matrix of _kernel_vec_distances, [B11 B22 B33 B44 B12 B13 B14 B23 B24 B34] over the control
// point pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); entries 60..65: the squared distances of the control points themselves
__device__ __forceinline__ int pair_lo(int p) { return p < 3 ? 0 : (p < 5 ? 1 : 2); }
__device__ __forceinline__ int pair_hi(int p) { return p < 3 ? p + 1 : (p < 5 ? p - 1 : 3); }
__device__ inline void kernel_distances(EpnpShared& sh, const double* mean, int t) {
  if (t < 60) {
    const int p = t / 10, col = t % 10;
    const int l = pair_lo(p), r = pair_hi(p);
    const int i = col < 4 ? col : pair_lo(col - 4), j = col < 4 ? col : pair_hi(col - 4);
    const double* ki = sh.kern[i];
    const double* kj = sh.kern[j];
    const double d0 = (ki[3 * l] - ki[3 * r]) * (kj[3 * l] - kj[3 * r]);
    const double d1 = (ki[3 * l + 1] - ki[3 * r + 1]) * (kj[3 * l + 1] - kj[3 * r + 1]);
    const double d2 = (ki[3 * l + 2] - ki[3 * r + 2]) * (kj[3 * l + 2] - kj[3 * r + 2]);
    const double v = (d0 + d1) + d2;
    sh.Lm[p][col] = col < 4 ? v : 2.0 * v;
  } else if (t < 66) {
    const int p = t - 60;
    const int l = pair_lo(p), r = pair_hi(p);
    double w[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)      // the control points as the reference holds them: unit axis + centroid
      w[c] = (((l == c) ? 1.0 : 0.0) + mean[c]) - (((r == c) ? 1.0 : 0.0) + mean[c]);
    sh.rhs[p] = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  }
}

// coefficients of the four kernel vectors for case `variant` (1..3) -- _find_null_space_coords_1/2/3
__device__ inline void null_space_coords(int variant, const EpnpShared& sh, double* beta) {
  double rhs[6];
#pragma unroll
  for (int p = 0; p < 6; ++p) rhs[p] = sh.rhs[p];
  const double (*Lm)[10] = sh.Lm;
  beta[0] = 0.0; beta[1] = 0.0; beta[2] = 0.0; beta[3] = 0.0;
  if (variant == 1) {
    double A[6][4], b[4];
#pragma unroll
    for (int p = 0; p < 6; ++p) { A[p][0] = Lm[p][0]; A[p][1] = Lm[p][4]; A[p][2] = Lm[p][5]; A[p][3] = Lm[p][6]; }
    lstsq6<4>(A, rhs, b);
    const double sg = (b[0] >= 0.0) ? 1.0 : -1.0;
    const double den = fmax(sqrt(b[0] * sg), kEps);
#pragma unroll
    for (int i = 0; i < 4; ++i) beta[i] = (b[i] * sg) / den;
  } else if (variant == 2) {
    double A[6][3], b[3];
#pragma unroll
    for (int p = 0; p < 6; ++p) { A[p][0] = Lm[p][0]; A[p][1] = Lm[p][4]; A[p][2] = Lm[p][1]; }
    lstsq6<3>(A, rhs, b);
    beta[0] = sqrt(fabs(b[0])) * ((b[1] >= 0.0) ? 1.0 : -1.0);
    beta[1] = sqrt(fabs(b[2])) * (((b[0] >= 0.0) == (b[2] >= 0.0)) ? 1.0 : 0.0);
  } else {
    double A[6][5], b[5];
#pragma unroll
    for (int p = 0; p < 6; ++p) { A[p][0] = Lm[p][0]; A[p][1] = Lm[p][4]; A[p][2] = Lm[p][1]; A[p][3] = Lm[p][5]; A[p][4] = Lm[p][7]; }
    lstsq6<5>(A, rhs, b);
    beta[0] = sqrt(fabs(b[0])) * ((b[1] >= 0.0) ? 1.0 : -1.0);
    beta[1] = sqrt(fabs(b[2])) * (((b[0] >= 0.0) == (b[2] >= 0.0)) ? 1.0 : 0.0);
    beta[2] = b[3] / fmax(beta[0], kEps);
  }
}

// The solver, called by all 256 threads of a workgroup with uniform arguments; x (N,3), y (N,2), w (N) or NULL.  Every
// thread returns the same `best` (candidate index, the key into sh.R / sh.T / sh.cc / sh.sc), err_2d, err_3d and validity.
__device__ __forceinline__ bool epnp_block(EpnpShared& sh, const double* x, const double* y, const uint8_t* w, int N, bool skip_quadratic,
                                  double* mean, int& best, double& err_2d, double& err_3d) {
  const int tid = threadIdx.x;
  const int nc = skip_quadratic ? 1 : 4;
  best = 0; err_2d = INFINITY; err_3d = INFINITY;
  // 1 -- centroid
  double cnt;
  {
    double acc[4] = {0.0, 0.0, 0.0, 0.0}, out[4];
    for (int n = tid; n < N; n += 256) {
      if (w && !w[n]) continue;
      acc[0] = acc[0] + x[3 * (size_t)n]; acc[1] = acc[1] + x[3 * (size_t)n + 1]; acc[2] = acc[2] + x[3 * (size_t)n + 2];
      acc[3] = acc[3] + 1.0;
    }
    block_tree_sum<4>(sh.red, acc, out);
    cnt = out[3];
    const double den = fmax(cnt, kEps);
    mean[0] = out[0] / den; mean[1] = out[1] / den; mean[2] = out[2] / den;
  }
  if (cnt < 4.0) return false;                       // (uniform: every thread holds the same count)
  // 2 -- the sums of a_j a_k {1, u, v, u^2 + v^2} and of a_j
  {
    double acc[44];
#pragma unroll
    for (int i = 0; i < 44; ++i) acc[i] = 0.0;
    for (int n = tid; n < N; n += 256) {
      if (w && !w[n]) continue;
      double a[4];
      alphas_of(x, (size_t)n, mean, a);
      const double u = y[2 * (size_t)n], v = y[2 * (size_t)n + 1];
      const double q = u * u + v * v;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int k = j; k < 4; ++k) {
          const double p = a[j] * a[k];
          acc[pair4(j, k)] = acc[pair4(j, k)] + p;
          acc[10 + pair4(j, k)] = acc[10 + pair4(j, k)] + p * u;
          acc[20 + pair4(j, k)] = acc[20 + pair4(j, k)] + p * v;
          acc[30 + pair4(j, k)] = acc[30 + pair4(j, k)] + p * q;
        }
        acc[40 + j] = acc[40 + j] + a[j];
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      double out[11];
      block_tree_sum<11>(sh.red, acc + 11 * g, out);
      if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 11; ++i) sh.sums[11 * g + i] = out[i];
      }
    }
  }
  __syncthreads();
  if (tid < 144) {
    const int r = tid / 12, c = tid % 12;
    const int p = pair4_any(r / 3, c / 3), cr = r % 3, cq = c % 3;
    double val;
    if (cr == 2 && cq == 2) val = sh.sums[30 + p];
    else if (cr == 2 || cq == 2) val = -sh.sums[((cr + cq == 2) ? 10 : 20) + p];      // (0,2), (2,0): -u; (1,2), (2,1): -v
    else val = (cr == cq) ? sh.sums[p] : 0.0;
    sh.G[r][c] = val;
  }
  __syncthreads();
  // 3 -- cyclic Jacobi on the first wavefront: lane g of a group of 16 holds row g of the matrix and of V
  if (tid < 64) {
    const int g = tid & 15;
    const int rg = g < 12 ? g : 0;
    double a[12], v[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) { a[j] = sh.G[rg][j]; v[j] = (j == g) ? 1.0 : 0.0; }
    // (jacobi_rows<12, 16, kSweeps12> of jacobi.hpp is this loop.  It is written out here because through the helper
    //  epnp_solve_kernel came out 290 instructions longer and 1.1 % slower: DESIGN.md section 23)
    for (int sw = 0; sw < kSweeps12; ++sw) {
#pragma unroll
      for (int p = 0; p < 11; ++p) {
#pragma unroll
        for (int q = p + 1; q < 12; ++q) {
          const double app = shfl16(a[p], p), aqq = shfl16(a[q], q), apq = shfl16(a[q], p);
          double c, s;
          jacobi_cs(app, aqq, apq, c, s);
          { const double cp = a[p], cq = a[q]; a[p] = c * cp - s * cq; a[q] = s * cp + c * cq; }
          double rp[12], rq[12];
#pragma unroll
          for (int j = 0; j < 12; ++j) { rp[j] = shfl16(a[j], p); rq[j] = shfl16(a[j], q); }
          if (g == p) {
#pragma unroll
            for (int j = 0; j < 12; ++j) a[j] = c * rp[j] - s * rq[j];
          } else if (g == q) {
#pragma unroll
            for (int j = 0; j < 12; ++j) a[j] = s * rp[j] + c * rq[j];
          }
          { const double vp = v[p], vq = v[q]; v[p] = c * vp - s * vq; v[q] = s * vp + c * vq; }
        }
      }
    }
    double nb[4];
    smallest_by_rank<12, 4, 16, false>(a, v, nb);
    // the sign of an eigenvector is the solver's choice, and case 3 depends on it (it divides by clamp(coord_0, 1e-9), and
    // coord_0 carries the sign of B12): the component of largest magnitude, the first such, is made positive
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      double top = 0.0, mag = -1.0;
#pragma unroll
      for (int j = 0; j < 12; ++j) {
        const double c = shfl16(nb[k], j);
        if (fabs(c) > mag) { mag = fabs(c); top = c; }
      }
      nb[k] = (top < 0.0) ? -nb[k] : nb[k];
    }
    if (tid < 12) {
#pragma unroll
      for (int k = 0; k < 4; ++k) sh.kern[k][tid] = nb[k];
    }
  }
  __syncthreads();
  if (!skip_quadratic) {
    kernel_distances(sh, mean, tid);
    __syncthreads();
  }
  // 4 -- thread k is candidate k
  if (tid < nc) {
    double beta[4] = {1.0, 0.0, 0.0, 0.0};
    if (tid > 0) null_space_coords(tid, sh, beta);
    double c[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int b = 0; b < 3; ++b)
        c[j][b] = ((sh.kern[0][3 * j + b] * beta[0] + sh.kern[1][3 * j + b] * beta[1]) + sh.kern[2][3 * j + b] * beta[2]) +
                  sh.kern[3][3 * j + b] * beta[3];
    const double* A1 = sh.sums + 40;
    const double den = fmax(cnt, kEps);
    const double mz = (((A1[0] * c[0][2] + A1[1] * c[1][2]) + A1[2] * c[2][2]) + A1[3] * c[3][2]) / den;
    const double flip = (mz < 0.0) ? -1.0 : 1.0;
    double ymu[3], C[9], R[9];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int b = 0; b < 3; ++b) c[j][b] = c[j][b] * flip;
#pragma unroll
    for (int b = 0; b < 3; ++b) ymu[b] = (((A1[0] * c[0][b] + A1[1] * c[1][b]) + A1[2] * c[2][b]) + A1[3] * c[3][b]) / den;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b)
        C[3 * a + b] = ((((sh.sums[pair4_any(a, 0)] * c[0][b] + sh.sums[pair4_any(a, 1)] * c[1][b]) + sh.sums[pair4_any(a, 2)] * c[2][b]) +
                         sh.sums[pair4_any(a, 3)] * c[3][b]) - A1[a] * ymu[b]) / den;
    const double xcov = ((sh.sums[pair4(0, 0)] + sh.sums[pair4(1, 1)]) + sh.sums[pair4(2, 2)]) / den;
    const double tr = kabsch3(C, R);
    const double s = tr / fmax(xcov, kEps);
    const double sc = fmax(s, kEps);
#pragma unroll
    for (int b = 0; b < 3; ++b)
      sh.T[tid][b] = (ymu[b] - s * ((mean[0] * R[b] + mean[1] * R[3 + b]) + mean[2] * R[6 + b])) / sc;
#pragma unroll
    for (int i = 0; i < 9; ++i) sh.R[tid][i] = R[i];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int b = 0; b < 3; ++b) sh.cc[tid][3 * j + b] = c[j][b];
    sh.sc[tid] = sc;
  }
  __syncthreads();
  // 5 -- the errors of the candidates
  double e2[4], e3[4];
  {
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, out[8];
    for (int n = tid; n < N; n += 256) {
      if (w && !w[n]) continue;
      double a[4];
      alphas_of(x, (size_t)n, mean, a);
      const double x0 = x[3 * (size_t)n], x1 = x[3 * (size_t)n + 1], x2 = x[3 * (size_t)n + 2];
      const double u = y[2 * (size_t)n], v = y[2 * (size_t)n + 1];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k >= nc) continue;
        const double* R = sh.R[k];
        const double* cc = sh.cc[k];
        double xr[3], d3 = 0.0;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          xr[b] = ((x0 * R[b] + x1 * R[3 + b]) + x2 * R[6 + b]) + sh.T[k][b];
          const double xc = (((a[0] * cc[b] + a[1] * cc[3 + b]) + a[2] * cc[6 + b]) + a[3] * cc[9 + b]) / sh.sc[k];
          const double d = xr[b] - xc;
          d3 = (b == 0) ? d * d : d3 + d * d;
        }
        const double z = fmax(xr[2], kEps);
        const double du = u - xr[0] / z, dw = v - xr[1] / z;
        acc[k] = acc[k] + sqrt(du * du + dw * dw);
        acc[4 + k] = acc[4 + k] + d3;
      }
    }
    block_tree_sum<8>(sh.red, acc, out);
    const double den = fmax(cnt, kEps);
#pragma unroll
    for (int k = 0; k < 4; ++k) { e2[k] = out[k] / den; e3[k] = out[4 + k] / den; }
  }
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k >= nc) continue;
    bool fin = isfinite(e2[k]) && isfinite(e3[k]) && isfinite(sh.sc[k]);
    for (int i = 0; i < 9; ++i) fin = fin && isfinite(sh.R[k][i]);
    for (int i = 0; i < 3; ++i) fin = fin && isfinite(sh.T[k][i]);
    ok = ok && fin;
    if (k == 0 || e2[k] < err_2d) { best = k; err_2d = e2[k]; err_3d = e3[k]; }      // the first minimum
  }
  if (!ok) { best = 0; err_2d = INFINITY; err_3d = INFINITY; return false; }
  return true;
}

// support of pose P (registers, the same in every thread) over the candidates of one frame; om: where to store the mask, or NULL
__device__ __forceinline__ void score_block(double (*red)[256], const double* P, const double* xf, const double* X, const uint8_t* mf, int N,
                                   double thr_sq, uint8_t* om, int& count, double& sum) {
  double acc[2] = {0.0, 0.0}, out[2];
  for (int n = threadIdx.x; n < N; n += 256) {
    double e = 0.0;
    const bool in = (!mf || mf[n]) &&
                    point_error(P, X[3 * (size_t)n], X[3 * (size_t)n + 1], X[3 * (size_t)n + 2], xf[2 * (size_t)n], xf[2 * (size_t)n + 1], thr_sq, e);
    acc[0] = acc[0] + (in ? 1.0 : 0.0);
    acc[1] = acc[1] + (in ? e : 0.0);
    if (om) om[n] = in ? 1 : 0;
  }
  block_tree_sum<2>(red, acc, out);
  count = (int)out[0];
  sum = out[1];
}

__global__ __launch_bounds__(256) void epnp_solve_kernel(const double* __restrict__ x, int x_shared, const double* __restrict__ y,
                                                        const uint8_t* __restrict__ weight, int N, int skip_quadratic,
                                                        double* __restrict__ outR, double* __restrict__ outT,
                                                        double* __restrict__ out_e2, double* __restrict__ out_e3,
                                                        double* __restrict__ out_xcam, int32_t* __restrict__ out_variant,
                                                        uint8_t* __restrict__ out_valid) {
  __shared__ EpnpShared sh;
  const size_t b = blockIdx.x;
  const int tid = threadIdx.x;
  const double* xb = x_shared ? x : x + b * N * 3;
  const double* yb = y + b * N * 2;
  const uint8_t* wb = weight ? weight + b * N : nullptr;
  double mean[3], e2, e3;
  int best;
  const bool ok = epnp_block(sh, xb, yb, wb, N, skip_quadratic != 0, mean, best, e2, e3);
  if (tid < 9) outR[b * 9 + tid] = ok ? sh.R[best][tid] : ((tid % 4 == 0) ? 1.0 : 0.0);
  if (tid < 3) outT[b * 3 + tid] = ok ? sh.T[best][tid] : 0.0;
  if (tid == 0) { out_e2[b] = e2; out_e3[b] = e3; out_variant[b] = best; out_valid[b] = ok ? 1 : 0; }
  if (out_xcam) {
    double* xc = out_xcam + b * N * 3;
    for (int n = tid; n < N; n += 256) {
      double r[3] = {0.0, 0.0, 0.0};
      if (ok && (!wb || wb[n])) {
        double a[4];
        alphas_of(xb, (size_t)n, mean, a);
        const double* cc = sh.cc[best];
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] = (((a[0] * cc[c] + a[1] * cc[3 + c]) + a[2] * cc[6 + c]) + a[3] * cc[9 + c]) / sh.sc[best];
      }
      xc[3 * (size_t)n] = r[0]; xc[3 * (size_t)n + 1] = r[1]; xc[3 * (size_t)n + 2] = r[2];
    }
  }
}

// grid = num_frames * num_poses
__global__ __launch_bounds__(256) void pose_score_kernel(const double* __restrict__ poses, const double* __restrict__ x,
                                                        const double* __restrict__ X, const uint8_t* __restrict__ mask,
                                                        const double* __restrict__ thr_sq, int L, int N,
                                                        int32_t* __restrict__ counts, double* __restrict__ sums,
                                                        uint8_t* __restrict__ out_masks) {
  __shared__ double red[2][256];
  const size_t slot = blockIdx.x, f = slot / L;
  double P[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) P[i] = poses[slot * 12 + i];
  int c;
  double s;
  score_block(red, P, x + f * N * 2, X, mask ? mask + f * N : nullptr, N, thr_sq[f], out_masks ? out_masks + slot * N : nullptr, c, s);
  if (threadIdx.x == 0) { counts[slot] = c; sums[slot] = s; }
}

// (the inlier mask is read back by the workgroup that wrote it: no __restrict__ on it)
__global__ __launch_bounds__(256) void epnp_lo_kernel(const double* __restrict__ x, const double* __restrict__ X,
                                                     const uint8_t* __restrict__ mask, const double* __restrict__ thr_sq, int N,
                                                     int max_rounds, double* __restrict__ pose, int32_t* __restrict__ num_inliers,
                                                     double* __restrict__ residual_sum, uint8_t* inlier_mask) {
  __shared__ EpnpShared sh;
  const size_t f = blockIdx.x;
  const int tid = threadIdx.x;
  if (num_inliers[f] <= 0) return;                   // nothing found: untouched
  const double* xf = x + f * N * 2;
  const uint8_t* mf = mask ? mask + f * N : nullptr;
  uint8_t* om = inlier_mask + f * N;
  const double thr = thr_sq[f];
  double P[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) P[i] = pose[f * 12 + i];
  __syncthreads();                                   // (every thread has read num_inliers and the pose before anything is stored)
  int cnt;
  double sum;
  score_block(sh.red, P, xf, X, mf, N, thr, om, cnt, sum);          // round 0: the baseline, in this file's arithmetic
  for (int round = 0; round < max_rounds; ++round) {
    if (cnt < kLoMinInliers) break;
    __syncthreads();                                 // the mask this workgroup stored is what it reads now
    double mean[3], e2, e3;
    int best;
    if (!epnp_block(sh, X, xf, om, N, false, mean, best, e2, e3)) break;
    double Q[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) Q[4 * i + j] = sh.R[best][3 * j + i];     // x R + T  ->  R^T X + T
      Q[4 * i + 3] = sh.T[best][i];
    }
    int c2;
    double s2;
    score_block(sh.red, Q, xf, X, mf, N, thr, nullptr, c2, s2);
    if (!(c2 > cnt || (c2 == cnt && s2 < sum))) break;
#pragma unroll
    for (int i = 0; i < 12; ++i) P[i] = Q[i];
    score_block(sh.red, P, xf, X, mf, N, thr, om, cnt, sum);        // the same arithmetic again, now storing the mask
  }
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < 12; ++i) pose[f * 12 + i] = P[i];
    num_inliers[f] = cnt; residual_sum[f] = sum;
  }
}

}  // namespace vgg

using namespace vgg;

extern "C" {

int vggp_epnp_solve(const double* x, int x_shared, const double* y, const uint8_t* weight, long num_problems, int num_points,
                    int skip_quadratic, double* out_R, double* out_T, double* out_err_2d, double* out_err_3d, double* out_x_cam,
                    int32_t* out_variant, uint8_t* out_valid, void* stream) {
  if (num_problems < 0 || num_points < 4) return VGG_ERR_INVALID_ARGUMENT;
  if (num_problems == 0) return VGG_OK;
  if (!x || !y || !out_R || !out_T || !out_err_2d || !out_err_3d || !out_variant || !out_valid) return VGG_ERR_INVALID_ARGUMENT;
  if (num_problems > 2147483647L) return VGG_ERR_UNSUPPORTED;
  epnp_solve_kernel<<<dim3((unsigned)num_problems), 256, 0, (hipStream_t)stream>>>(
      x, x_shared, y, weight, num_points, skip_quadratic, out_R, out_T, out_err_2d, out_err_3d, out_x_cam, out_variant, out_valid);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vggp_pose_score(const double* poses, const double* points2D_normalized, const double* points3D, const uint8_t* candidate_mask,
                    const double* max_error_sq, long num_frames, int num_poses, int num_points, int32_t* out_counts,
                    double* out_residual_sums, uint8_t* out_masks, void* stream) {
  if (num_frames < 0 || num_poses <= 0 || num_points <= 0) return VGG_ERR_INVALID_ARGUMENT;
  if (num_frames == 0) return VGG_OK;
  if (!poses || !points2D_normalized || !points3D || !max_error_sq || !out_counts || !out_residual_sums)
    return VGG_ERR_INVALID_ARGUMENT;
  if (num_frames > 2147483647L / num_poses) return VGG_ERR_UNSUPPORTED;
  pose_score_kernel<<<dim3((unsigned)(num_frames * num_poses)), 256, 0, (hipStream_t)stream>>>(
      poses, points2D_normalized, points3D, candidate_mask, max_error_sq, num_poses, num_points, out_counts, out_residual_sums,
      out_masks);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vggp_epnp_lo(const double* points2D_normalized, const double* points3D, const uint8_t* candidate_mask,
                 const double* max_error_sq, long num_frames, int num_points, int max_rounds, double* pose, int32_t* num_inliers,
                 double* residual_sum, uint8_t* inlier_mask, void* stream) {
  if (num_frames < 0 || num_points < 4 || max_rounds < 0) return VGG_ERR_INVALID_ARGUMENT;
  if (num_frames == 0) return VGG_OK;
  if (!points2D_normalized || !points3D || !max_error_sq || !pose || !num_inliers || !residual_sum || !inlier_mask)
    return VGG_ERR_INVALID_ARGUMENT;
  if (num_frames > 2147483647L) return VGG_ERR_UNSUPPORTED;
  epnp_lo_kernel<<<dim3((unsigned)num_frames), 256, 0, (hipStream_t)stream>>>(
      points2D_normalized, points3D, candidate_mask, max_error_sq, num_points, max_rounds, pose, num_inliers, residual_sum,
      inlier_mask);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

}  // extern "C"
