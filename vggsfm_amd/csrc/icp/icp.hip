// ICP on the uniform grid of the nearest-neighbour library, for gfx950: the entries of vggsfm_amd_icp.h.  A parity file:
// built with -ffp-contract=off, every expression in the header's order (tests/icp_cases.py restates it in NumPy over all
// pairs, with no grid).  The grid walk is csrc/nn/nn_grid.hpp's, the one copy nn.hip uses.
#include <math.h>

#include <type_traits>

#include "../jacobi.hpp"
#include "../nn/nn_grid.hpp"
#include "vggsfm_amd_icp.h"

namespace vgg {

constexpr long kMaxCells = 33554432;             // VGGN_MAX_CELLS of vggsfm_amd_nn.h
constexpr int kSums = 38;                        // the double words of a workspace row
constexpr int kWaves = VGGI_BLOCK / 64;

struct StepOptions {
  double r, r2, loss_scale;
  int metric, estimate_scale, loss;
};

struct Transform {
  double s, R[9], t[3], c[3];
};

// one residual row: H += (w J)(J)^T (upper triangle), g += (w J) r
__device__ __forceinline__ void add_row(double* acc, const double* J, double r, double w) {
  int k = 0;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const double wj = w * J[i];
#pragma unroll
    for (int j = i; j < 7; ++j) {
      acc[k] = acc[k] + wj * J[j];
      ++k;
    }
    acc[28 + i] = acc[28 + i] + wj * r;
  }
}

// steps 3 to 6 of the header for a pair (x, y, n); returns false when the pair is dropped
__device__ __forceinline__ bool add_pair(double* acc, const Transform& T, const StepOptions& o, double x0, double x1, double x2,
                                         double y0, double y1, double y2, double n0, double n1, double n2, bool have_normal) {
  if (have_normal && !finite3(n0, n1, n2)) return false;
  const double e0 = x0 - y0, e1 = x1 - y1, e2 = x2 - y2;
  const double z0 = x0 - T.c[0], z1 = x1 - T.c[1], z2 = x2 - T.c[2];
  double rho, R2, rp = 0.0;
  if (o.metric == 1) {
    rp = dot3(n0, n1, n2, e0, e1, e2);
    rho = fabs(rp);
    R2 = rp * rp;
  } else {
    R2 = dot3(e0, e1, e2, e0, e1, e2);
    rho = sqrt(R2);
  }
  double w = 1.0;
  if (o.loss == 1) {
    w = rho <= o.loss_scale ? 1.0 : o.loss_scale / rho;
  } else if (o.loss == 2) {
    const double q = rho / o.loss_scale, v = 1.0 - (q * q);
    w = rho < o.loss_scale ? v * v : 0.0;
  }
  if (o.metric == 1) {
    const double J[7] = {z1 * n2 - z2 * n1, z2 * n0 - z0 * n2, z0 * n1 - z1 * n0, n0, n1, n2,
                         o.estimate_scale ? dot3(n0, n1, n2, z0, z1, z2) : 0.0};
    add_row(acc, J, rp, w);
  } else {
    const double l0 = o.estimate_scale ? z0 : 0.0, l1 = o.estimate_scale ? z1 : 0.0, l2 = o.estimate_scale ? z2 : 0.0;
    const double Ja[7] = {0.0, z2, -z1, 1.0, 0.0, 0.0, l0}, Jb[7] = {-z2, 0.0, z0, 0.0, 1.0, 0.0, l1},
                 Jc[7] = {z1, -z0, 0.0, 0.0, 0.0, 1.0, l2};
    add_row(acc, Ja, e0, w);
    add_row(acc, Jb, e1, w);
    add_row(acc, Jc, e2, w);
  }
  acc[35] = acc[35] + w;
  acc[36] = acc[36] + w * R2;
  acc[37] = acc[37] + R2;
  return true;
}

struct PointTarget {
  const double* points;
  const int32_t* index;
  const int32_t* cell_start;
  const double* normals;
  int n;
};

struct MeshTarget {
  const double* vertices;
  const int32_t* faces;
  const int32_t* cell_faces;
  const int32_t* cell_start;
  int V, F, num_pairs;
};

// the winner of vggn_nearest_point's rule and its point; -1: none
__device__ __forceinline__ int nearest_in(const PointTarget& tg, const Grid& g, double q0, double q1, double q2, double r, double r2,
                                          double& y0, double& y1, double& y2) {
  int bi = -1;
  if (tg.n <= 0) return bi;
  double best = INFINITY;
  int lo0, hi0, lo1, hi1, lo2, hi2;
  axis_range(q0, r, g.ox, g.cell, g.d0, lo0, hi0);
  axis_range(q1, r, g.oy, g.cell, g.d1, lo1, hi1);
  axis_range(q2, r, g.oz, g.cell, g.d2, lo2, hi2);
  for (int c2 = lo2; c2 <= hi2; ++c2) {
    for (int c1 = lo1; c1 <= hi1; ++c1) {
      const long row = ((long)c2 * g.d1 + c1) * g.d0;
      const int s = max(tg.cell_start[row + lo0], 0), e = min(tg.cell_start[row + hi0 + 1], tg.n);
      for (int k = s; k < e; ++k) {
        const double p0 = tg.points[3 * (long)k], p1 = tg.points[3 * (long)k + 1], p2 = tg.points[3 * (long)k + 2];
        const double dx = q0 - p0, dy = q1 - p1, dz = q2 - p2;
        const double d2 = ((dx * dx) + (dy * dy)) + dz * dz;
        if (!(d2 <= r2)) continue;
        const int idx = tg.index[k];
        if (bi < 0 || d2 < best || (d2 == best && idx < bi)) {
          best = d2;
          bi = idx;
          y0 = p0; y1 = p1; y2 = p2;
        }
      }
    }
  }
  return bi;
}

// the winner of vggn_nearest_face's rule, its closest point and its unit normal; -1: none
__device__ __forceinline__ int nearest_in(const MeshTarget& tg, const Grid& g, double q0, double q1, double q2, double r, double r2,
                                          double& y0, double& y1, double& y2, double& n0, double& n1, double& n2) {
  int bf = -1;
  if (tg.num_pairs <= 0 || tg.F <= 0) return bf;
  double best = INFINITY;
  Triangle bt;
  int lo0, hi0, lo1, hi1, lo2, hi2;
  axis_range(q0, r, g.ox, g.cell, g.d0, lo0, hi0);
  axis_range(q1, r, g.oy, g.cell, g.d1, lo1, hi1);
  axis_range(q2, r, g.oz, g.cell, g.d2, lo2, hi2);
  for (int c2 = lo2; c2 <= hi2; ++c2) {
    for (int c1 = lo1; c1 <= hi1; ++c1) {
      const long row = ((long)c2 * g.d1 + c1) * g.d0;
      const int s = max(tg.cell_start[row + lo0], 0), e = min(tg.cell_start[row + hi0 + 1], tg.num_pairs);
      for (int k = s; k < e; ++k) {
        const int f = tg.cell_faces[k];
        Triangle t;
        if (f < 0 || f >= tg.F || f == bf || !face_vertices(tg.vertices, tg.V, tg.faces, f, t)) continue;
        double x0, x1, x2;
        closest_point(t, q0, q1, q2, x0, x1, x2);
        const double dx = q0 - x0, dy = q1 - x1, dz = q2 - x2;
        const double d2 = ((dx * dx) + (dy * dy)) + dz * dz;
        if (!(d2 <= r2)) continue;
        if (bf < 0 || d2 < best || (d2 == best && f < bf)) {
          best = d2;
          bf = f;
          bt = t;
          y0 = x0; y1 = x1; y2 = x2;
        }
      }
    }
  }
  if (bf >= 0) {
    const double ab0 = bt.b0 - bt.a0, ab1 = bt.b1 - bt.a1, ab2 = bt.b2 - bt.a2, ac0 = bt.c0 - bt.a0, ac1 = bt.c1 - bt.a1,
                 ac2 = bt.c2 - bt.a2;
    const double u0 = ab1 * ac2 - ab2 * ac1, u1 = ab2 * ac0 - ab0 * ac2, u2 = ab0 * ac1 - ab1 * ac0;
    const double len = sqrt(dot3(u0, u1, u2, u0, u1, u2));
    n0 = u0 / len; n1 = u1 / len; n2 = u2 / len;
  }
  return bf;
}

__device__ __forceinline__ void load_transform(const double* __restrict__ state, Transform& T) {
  T.s = state[2];
#pragma unroll
  for (int i = 0; i < 9; ++i) T.R[i] = state[3 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) { T.t[i] = state[12 + i]; T.c[i] = state[15 + i]; }
}

// VGGI_GROUPS workgroups of VGGI_BLOCK lanes; every lane reaches the butterflies (no early return past the status test, which
// is uniform over the launch).
template <typename Target>
__global__ __launch_bounds__(VGGI_BLOCK) void icp_step_kernel(const double* __restrict__ source, const int32_t* __restrict__ visit, int m,
                                                              Target tg, Grid g, const double* __restrict__ state, StepOptions o,
                                                              double* __restrict__ ws, int32_t* __restrict__ out_index) {
  if (state[0] != (double)VGGI_RUNNING) return;
  __shared__ double part[kWaves][VGGI_WORDS];
  __shared__ long long part_count[kWaves];
  Transform T;
  load_transform(state, T);
  double acc[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
  int count = 0;
  for (long j = (long)blockIdx.x * VGGI_BLOCK + threadIdx.x; j < m; j += (long)VGGI_BLOCK * VGGI_GROUPS) {
    const int qi = visit[j];
    if (qi < 0 || qi >= m) continue;
    const double p0 = source[3 * (long)qi], p1 = source[3 * (long)qi + 1], p2 = source[3 * (long)qi + 2];
    const double x0 = (T.s * (((T.R[0] * p0) + (T.R[1] * p1)) + T.R[2] * p2)) + T.t[0];
    const double x1 = (T.s * (((T.R[3] * p0) + (T.R[4] * p1)) + T.R[5] * p2)) + T.t[1];
    const double x2 = (T.s * (((T.R[6] * p0) + (T.R[7] * p1)) + T.R[8] * p2)) + T.t[2];
    int winner = -1;
    bool kept = false;
    if (finite3(x0, x1, x2)) {
      double y0 = 0.0, y1 = 0.0, y2 = 0.0, n0 = 0.0, n1 = 0.0, n2 = 0.0;
      bool have_normal;
      if constexpr (std::is_same<Target, PointTarget>::value) {
        winner = nearest_in(tg, g, x0, x1, x2, o.r, o.r2, y0, y1, y2);
        have_normal = tg.normals != nullptr;
        if (winner >= 0 && have_normal) {
          const bool ok = winner < tg.n;
          n0 = ok ? tg.normals[3 * (long)winner] : NAN;
          n1 = ok ? tg.normals[3 * (long)winner + 1] : NAN;
          n2 = ok ? tg.normals[3 * (long)winner + 2] : NAN;
        }
      } else {
        winner = nearest_in(tg, g, x0, x1, x2, o.r, o.r2, y0, y1, y2, n0, n1, n2);
        have_normal = true;
      }
      if (winner >= 0) kept = add_pair(acc, T, o, x0, x1, x2, y0, y1, y2, n0, n1, n2, have_normal);
    }
    count += kept ? 1 : 0;
    if (out_index != nullptr) out_index[qi] = kept ? winner : -1;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  wave_reduce_scatter<kSums, 32>(acc, lane, kSums, 0, part[wave]);
  count = wave_sum_i(count);
  if (lane == 0) part_count[wave] = count;
  __syncthreads();
  const int w = threadIdx.x;
  if (w < kSums) {
    double s = part[0][w];
#pragma unroll
    for (int v = 1; v < kWaves; ++v) s = s + part[v][w];
    ws[(long)blockIdx.x * VGGI_WORDS + w] = s;
  } else if (w == kSums) {
    long long s = 0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) s += part_count[v];
    ((long long*)ws)[(long)blockIdx.x * VGGI_WORDS + w] = s;
  } else if (w == kSums + 1) {
    ((long long*)ws)[(long)blockIdx.x * VGGI_WORDS + w] = 0;
  }
}

// word `lane` of the workspace rows added in ascending group order -> total[lane] (LDS), lanes < VGGI_WORDS.  The loads of
// kBatch rows are issued before their additions (the additions wait on one another, the loads need not): same order, same bits.
__device__ __forceinline__ void sum_rows(const double* __restrict__ ws, double* total, int lane) {
  constexpr int kBatch = 32;
  static_assert(VGGI_GROUPS % kBatch == 0, "VGGI_GROUPS is a multiple of the load batch");
  if (lane < kSums) {
    double s = 0.0;
    for (int b = 0; b < VGGI_GROUPS; b += kBatch) {
      double v[kBatch];
#pragma unroll
      for (int k = 0; k < kBatch; ++k) v[k] = ws[(long)(b + k) * VGGI_WORDS + lane];
#pragma unroll
      for (int k = 0; k < kBatch; ++k) s = s + v[k];
    }
    total[lane] = s;
  } else if (lane == kSums) {
    const long long* wi = (const long long*)ws;
    long long s = 0;
#pragma unroll 16
    for (int b = 0; b < VGGI_GROUPS; ++b) s += wi[(long)b * VGGI_WORDS + lane];
    ((long long*)total)[lane] = s;
  } else if (lane == kSums + 1) {
    ((long long*)total)[lane] = 0;
  }
}

__global__ __launch_bounds__(64) void icp_sums_kernel(const double* __restrict__ ws, double* __restrict__ out) {
  __shared__ double total[VGGI_WORDS];
  const int lane = threadIdx.x;
  sum_rows(ws, total, lane);
  __syncthreads();
  if (lane < VGGI_WORDS) ((long long*)out)[lane] = ((const long long*)total)[lane];
}

struct UpdateOptions {
  double damping, rotation_tol, translation_tol, scale_tol;
  int estimate_scale, min_correspondences, history_rows;
};

__global__ __launch_bounds__(64) void icp_update_kernel(const double* __restrict__ ws, double* __restrict__ state, UpdateOptions o,
                                                        double* __restrict__ history) {
  if (state[0] != (double)VGGI_RUNNING) return;
  __shared__ double total[VGGI_WORDS];
  const int lane = threadIdx.x;
  sum_rows(ws, total, lane);
  __syncthreads();
  if (lane != 0) return;
  const long long count = ((const long long*)total)[kSums];
  if (count < (long long)o.min_correspondences) {
    state[0] = (double)VGGI_TOO_FEW;
    return;
  }
  const int n = o.estimate_scale ? 7 : 6;
  double H[7][7], d[7], b[7];
  {
    int k = 0;
    for (int i = 0; i < 7; ++i)
      for (int j = i; j < 7; ++j) H[i][j] = total[k++];
  }
  for (int i = 0; i < n; ++i) {
    if (!(H[i][i] > 0.0)) {
      state[0] = (double)VGGI_DEGENERATE;
      return;
    }
    d[i] = 1.0 / sqrt(H[i][i]);
  }
  double L[7][7];
  for (int j = 0; j < n; ++j) {
    double p = 1.0 + o.damping;
    for (int k = 0; k < j; ++k) p = p - L[j][k] * L[j][k];
    if (!(p > VGGI_PIVOT_MIN)) {
      state[0] = (double)VGGI_DEGENERATE;
      return;
    }
    L[j][j] = sqrt(p);
    for (int i = j + 1; i < n; ++i) {
      double a = (H[j][i] * d[j]) * d[i];          // A_ij with i > j: the upper triangle holds H_ji
      for (int k = 0; k < j; ++k) a = a - L[i][k] * L[j][k];
      L[i][j] = a / L[j][j];
    }
  }
  for (int i = 0; i < n; ++i) {
    double a = -(total[28 + i] * d[i]);
    for (int k = 0; k < i; ++k) a = a - L[i][k] * b[k];
    b[i] = a / L[i][i];
  }
  double delta[7];
  delta[6] = 0.0;
  for (int i = n - 1; i >= 0; --i) {
    double a = b[i];
    for (int k = i + 1; k < n; ++k) a = a - L[k][i] * delta[k];
    delta[i] = a / L[i][i];
  }
  for (int i = 0; i < n; ++i) delta[i] = delta[i] * d[i];
  const double w0 = delta[0], w1 = delta[1], w2 = delta[2], lambda = delta[6];
  const double th2 = dot3(w0, w1, w2, w0, w1, w2), th = sqrt(th2);
  double A, B;
  if (th2 < 1e-8) {
    A = 1.0 - th2 / 6.0;
    B = 0.5 - th2 / 24.0;
  } else {
    const double h = sin(0.5 * th);
    A = sin(th) / th;
    B = (2.0 * (h * h)) / th2;
  }
  const double w[3] = {w0, w1, w2};
  const double K[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
  double E[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) E[i][j] = ((i == j ? 1.0 : 0.0) + A * K[i][j]) + B * ((w[i] * w[j]) - (i == j ? th2 : 0.0));
  double R[3][3], t[3], c[3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) R[i][j] = state[3 + 3 * i + j];
    t[i] = state[12 + i];
    c[i] = state[15 + i];
  }
  const double u0 = t[0] - c[0], u1 = t[1] - c[1], u2 = t[2] - c[2];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) state[3 + 3 * i + j] = ((E[i][0] * R[0][j]) + (E[i][1] * R[1][j])) + E[i][2] * R[2][j];
    state[12 + i] = (c[i] + (1.0 + lambda) * dot3(E[i][0], E[i][1], E[i][2], u0, u1, u2)) + delta[3 + i];
  }
  state[2] = state[2] * (1.0 + lambda);
  const double nt = sqrt(dot3(delta[3], delta[4], delta[5], delta[3], delta[4], delta[5]));
  const double it = state[1];
  if (history != nullptr && it >= 0.0 && it < (double)o.history_rows) {
    double* row = history + (long)it * VGGI_HISTORY_WORDS;
    row[0] = (double)count;
    row[1] = total[35];
    row[2] = total[36];
    row[3] = total[37];
    row[4] = th;
    row[5] = nt;
    row[6] = lambda;
  }
  state[1] = it + 1.0;
  if (th <= o.rotation_tol && nt <= o.translation_tol && fabs(lambda) <= o.scale_tol) state[0] = (double)VGGI_CONVERGED;
}

struct Viewpoint {
  double p[3];
  int given;
};

// One lane per sorted grid point; two passes over its neighbours.
__global__ __launch_bounds__(256) void radius_normals_kernel(const double* __restrict__ grid_points, const int32_t* __restrict__ grid_index,
                                                             const int32_t* __restrict__ cell_start, int n, Grid g, double r, double r2,
                                                             int min_neighbors, Viewpoint vp, double* __restrict__ out_normal,
                                                             double* __restrict__ out_curvature, int32_t* __restrict__ out_count) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int oi = grid_index[i];
  if (oi < 0 || oi >= n) return;
  const double q0 = grid_points[3 * i], q1 = grid_points[3 * i + 1], q2 = grid_points[3 * i + 2];
  int count = 0;
  double nx = NAN, ny = NAN, nz = NAN, curv = NAN;
  if (finite3(q0, q1, q2)) {
    int lo0, hi0, lo1, hi1, lo2, hi2;
    axis_range(q0, r, g.ox, g.cell, g.d0, lo0, hi0);
    axis_range(q1, r, g.oy, g.cell, g.d1, lo1, hi1);
    axis_range(q2, r, g.oz, g.cell, g.d2, lo2, hi2);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    double C[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    double m0 = 0.0, m1 = 0.0, m2 = 0.0;
    for (int pass = 0; pass < 2; ++pass) {
      for (int c2 = lo2; c2 <= hi2; ++c2) {
        for (int c1 = lo1; c1 <= hi1; ++c1) {
          const long row = ((long)c2 * g.d1 + c1) * g.d0;
          const int s = max(cell_start[row + lo0], 0), e = min(cell_start[row + hi0 + 1], n);
          for (int k = s; k < e; ++k) {
            const double p0 = grid_points[3 * (long)k], p1 = grid_points[3 * (long)k + 1], p2 = grid_points[3 * (long)k + 2];
            const double dx = q0 - p0, dy = q1 - p1, dz = q2 - p2;
            const double d2 = ((dx * dx) + (dy * dy)) + dz * dz;
            if (!(d2 <= r2)) continue;
            if (pass == 0) {
              ++count;
              s0 = s0 + p0; s1 = s1 + p1; s2 = s2 + p2;
            } else {
              const double a0 = p0 - m0, a1 = p1 - m1, a2 = p2 - m2;
              C[0][0] = C[0][0] + a0 * a0; C[0][1] = C[0][1] + a0 * a1; C[0][2] = C[0][2] + a0 * a2;
              C[1][1] = C[1][1] + a1 * a1; C[1][2] = C[1][2] + a1 * a2; C[2][2] = C[2][2] + a2 * a2;
            }
          }
        }
      }
      if (pass == 0) {
        if (count < min_neighbors) break;
        m0 = s0 / count; m1 = s1 / count; m2 = s2 / count;
      }
    }
    if (count >= min_neighbors) {
      C[0][0] = C[0][0] / count; C[0][1] = C[0][1] / count; C[0][2] = C[0][2] / count;
      C[1][1] = C[1][1] / count; C[1][2] = C[1][2] / count; C[2][2] = C[2][2] / count;
      C[1][0] = C[0][1]; C[2][0] = C[0][2]; C[2][1] = C[1][2];
      double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
      jacobi_sym3<VGGI_NORMAL_SWEEPS, true>(C, V);
      const double l0 = C[0][0], l1 = C[1][1], l2 = C[2][2];
      const int b = (l1 < l0) ? ((l2 < l1) ? 2 : 1) : ((l2 < l0) ? 2 : 0);
      const double lb = b == 0 ? l0 : (b == 1 ? l1 : l2);
      double v0 = b == 0 ? V[0][0] : (b == 1 ? V[0][1] : V[0][2]);
      double v1 = b == 0 ? V[1][0] : (b == 1 ? V[1][1] : V[1][2]);
      double v2 = b == 0 ? V[2][0] : (b == 1 ? V[2][1] : V[2][2]);
      const double len = sqrt(dot3(v0, v1, v2, v0, v1, v2));
      v0 = v0 / len; v1 = v1 / len; v2 = v2 / len;
      bool flip;
      if (vp.given) flip = dot3(v0, v1, v2, vp.p[0] - q0, vp.p[1] - q1, vp.p[2] - q2) < 0.0;
      else flip = v0 != 0.0 ? v0 < 0.0 : (v1 != 0.0 ? v1 < 0.0 : v2 < 0.0);
      nx = flip ? -v0 : v0; ny = flip ? -v1 : v1; nz = flip ? -v2 : v2;
      curv = lb / ((l0 + l1) + l2);
    }
  }
  out_normal[3 * (long)oi] = nx;
  out_normal[3 * (long)oi + 1] = ny;
  out_normal[3 * (long)oi + 2] = nz;
  out_curvature[oi] = curv;
  out_count[oi] = count;
}

static bool step_options(double max_dist, double r2, int metric, int estimate_scale, int loss, double loss_scale, StepOptions& o) {
  if (!(max_dist > 0.0) || !(r2 >= 0.0) || (metric != 0 && metric != 1) || loss < 0 || loss > 2) return false;
  if (loss != 0 && !(loss_scale > 0.0)) return false;
  o = StepOptions{max_dist, r2, loss != 0 ? loss_scale : 1.0, metric, estimate_scale ? 1 : 0, loss};
  return true;
}

}  // namespace vgg

using namespace vgg;

extern "C" {

const char* vggi_build_arch(void) { return "gfx950"; }

int vggi_icp_step(const double* source, const int32_t* visit, int m, const double* grid_points, const int32_t* grid_index,
                  const int32_t* cell_start, int n, double ox, double oy, double oz, double cell, int d0, int d1, int d2,
                  const double* normals, const double* state, double max_dist, double r2, int metric, int estimate_scale,
                  int loss, double loss_scale, void* workspace, int32_t* out_index, void* stream) {
  Grid g;
  StepOptions o;
  if (!grid_argument(ox, oy, oz, cell, d0, d1, d2, kMaxCells, g) || n < 0 || m < 0 ||
      !step_options(max_dist, r2, metric, estimate_scale, loss, loss_scale, o))
    return VGG_ERR_INVALID_ARGUMENT;
  if (metric == 1 && !normals && n > 0) return VGG_ERR_INVALID_ARGUMENT;
  if (!state || !workspace || (m > 0 && (!source || !visit)) || (m > 0 && n > 0 && (!grid_points || !grid_index || !cell_start)))
    return VGG_ERR_INVALID_ARGUMENT;
  const PointTarget tg{grid_points, grid_index, cell_start, normals, n};
  icp_step_kernel<PointTarget><<<VGGI_GROUPS, VGGI_BLOCK, 0, (hipStream_t)stream>>>(source, visit, m, tg, g, state, o, (double*)workspace,
                                                                                   out_index);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vggi_icp_step_mesh(const double* source, const int32_t* visit, int m, const double* vertices, int num_vertices,
                       const int32_t* faces, int num_faces, const int32_t* cell_faces, const int32_t* cell_start,
                       int num_pairs, double ox, double oy, double oz, double cell, int d0, int d1, int d2,
                       const double* state, double max_dist, double r2, int metric, int estimate_scale, int loss,
                       double loss_scale, void* workspace, int32_t* out_index, void* stream) {
  Grid g;
  StepOptions o;
  if (!grid_argument(ox, oy, oz, cell, d0, d1, d2, kMaxCells, g) || num_vertices < 0 || num_faces < 0 || num_pairs < 0 || m < 0 ||
      !step_options(max_dist, r2, metric, estimate_scale, loss, loss_scale, o))
    return VGG_ERR_INVALID_ARGUMENT;
  const bool work = m > 0 && num_faces > 0 && num_pairs > 0;
  if (!state || !workspace || (m > 0 && (!source || !visit)) || (work && (!vertices || !faces || !cell_faces || !cell_start)))
    return VGG_ERR_INVALID_ARGUMENT;
  const MeshTarget tg{vertices, faces, cell_faces, cell_start, num_vertices, num_faces, num_pairs};
  icp_step_kernel<MeshTarget><<<VGGI_GROUPS, VGGI_BLOCK, 0, (hipStream_t)stream>>>(source, visit, m, tg, g, state, o, (double*)workspace,
                                                                                  out_index);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vggi_icp_sums(const void* workspace, void* out, void* stream) {
  if (!workspace || !out) return VGG_ERR_INVALID_ARGUMENT;
  icp_sums_kernel<<<1, 64, 0, (hipStream_t)stream>>>((const double*)workspace, (double*)out);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vggi_icp_update(const void* workspace, double* state, int estimate_scale, int min_correspondences, double damping,
                    double rotation_tol, double translation_tol, double scale_tol, double* history, int history_rows,
                    void* stream) {
  if (!workspace || !state || min_correspondences < 1 || !(damping >= 0.0) || rotation_tol != rotation_tol ||
      translation_tol != translation_tol || scale_tol != scale_tol || history_rows < 0 || (history_rows > 0 && !history))
    return VGG_ERR_INVALID_ARGUMENT;
  const UpdateOptions o{damping, rotation_tol, translation_tol, scale_tol, estimate_scale ? 1 : 0, min_correspondences,
                        history ? history_rows : 0};
  icp_update_kernel<<<1, 64, 0, (hipStream_t)stream>>>((const double*)workspace, state, o, history);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vggi_radius_normals(const double* grid_points, const int32_t* grid_index, const int32_t* cell_start, int n, double ox,
                        double oy, double oz, double cell, int d0, int d1, int d2, double radius, double r2,
                        int min_neighbors, const double* toward, double* out_normal, double* out_curvature,
                        int32_t* out_count, void* stream) {
  Grid g;
  if (!grid_argument(ox, oy, oz, cell, d0, d1, d2, kMaxCells, g) || n < 0 || !(radius > 0.0) || !(r2 >= 0.0) || min_neighbors < 1)
    return VGG_ERR_INVALID_ARGUMENT;
  Viewpoint vp{{0.0, 0.0, 0.0}, 0};
  if (toward) {
    for (int k = 0; k < 3; ++k) {
      if (!(toward[k] - toward[k] == 0.0)) return VGG_ERR_INVALID_ARGUMENT;
      vp.p[k] = toward[k];
    }
    vp.given = 1;
  }
  if (n == 0) return VGG_OK;
  if (!grid_points || !grid_index || !cell_start || !out_normal || !out_curvature || !out_count) return VGG_ERR_INVALID_ARGUMENT;
  radius_normals_kernel<<<div_up(n, 256), 256, 0, (hipStream_t)stream>>>(grid_points, grid_index, cell_start, n, g, radius, r2,
                                                                         min_neighbors, vp, out_normal, out_curvature, out_count);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

}  // extern "C"
