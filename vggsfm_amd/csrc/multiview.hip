// Masked multi-view DLT triangulation and the angle helpers around it, as entries of their own (gfx950).
//
// Replaces, one for one (include/vggsfm_amd_multiview.h):
//   vggsfm/utils/triangulation_helpers.py:27-131      triangulate_multi_view_point_batched
//   vggsfm/utils/triangulation_helpers.py:431-472     calculate_normalized_angular_error_batched
//   vggsfm/utils/triangulation_helpers.py:475-587     calculate_triangulation_angle{_batched,_exhaustive,}
//   vggsfm/utils/triangulation_helpers.py:648-725     local_refinement_tri (all B x lo_num solves in one launch)
// The reference expands the cameras per point (B,S,3,4), builds a (B,S,3,4) `terms` tensor and an (B,S*S) angle table.
// Here one LANE owns one point: it walks the S views, reads its observation (consecutive lanes read consecutive points of
// the (S,N,2) track layout: coalesced), adds the view's weighted 3x4 term into the 10 unique entries of the symmetric 4x4
// normal matrix in registers, solves for the smallest eigenvector with a cyclic Jacobi in registers and sweeps the views
// once more for the cheirality.  With one shared camera set the projection matrices and centres are wave-uniform (scalar
// loads); with per-group cameras every lane reads its own.  The angle pass is a second kernel: per point the maximum over
// the S(S-1)/2 unordered pairs (the expression is symmetric in the two cameras bit for bit, and a diagonal pair gives
// exactly 0: sqrt(r*r) == r), or the (B,S*S) table for the namesakes.
// This file is compiled with -ffp-contract=off (the reference's unfused arithmetic), triangulate.hip with contraction.
// Contraction is set per translation unit, so the helpers the two files share as headers (jacobi.hpp, tri_angle.hpp) are
// compiled under each file's own setting: one source, each file's rounding as it was.
// No atomics, no cross-lane arithmetic: a point's result does not depend on what else is in the launch.
#include "common.hpp"
#include "jacobi.hpp"
#include "tri_angle.hpp"
#include "../../include/vggsfm_amd_multiview.h"

namespace vgg {
namespace {

constexpr double kMvPi = 3.141592653589793;
constexpr double kMvEps = 1e-12;          // the eps default of calculate_triangulation_angle_batched (the reduced pass)

constexpr int kMvSweeps4 = 16;            // the 4x4 Jacobi of mv_solve_kernel: at most this many sweeps ...
constexpr double kMvTol4 = 1e-24;         // ... done at this ratio of the off-diagonal sum to the diagonal's

// triangulation_helpers.py:503-519: law of cosines on squared lengths, min(theta, pi - theta), degrees
__device__ __forceinline__ double mv_angle_deg(double r1, double r2, double bsq, double eps) {
  double den = 2.0 * sqrt(r1 * r2);
  double nom = r1 + r2 - bsq;
  if (den <= eps) { nom = 1.0; den = 1.0; }
  double c = nom / den;
  c = (c != c) ? c : fmin(fmax(c, -1.0), 1.0);          // torch.clamp keeps NaN
  double th = fabs(acos(c));
  th = (th != th) ? th : fmin(th, kMvPi - th);
  return th * (180.0 / kMvPi);
}

struct MvSolve {
  const double* cams;
  const void* tracks;
  const void* weights;
  const int64_t* weight_rows;
  long track_stride_q, track_stride_s, weight_stride_row, weight_stride_s, n;
  int group_div, weight_kind, S, zero_masked;
  double* out_points;
  uint8_t* out_invalid;
};

template <typename T> struct Vec2;
template <> struct Vec2<float> { using type = float2; };
template <> struct Vec2<double> { using type = double2; };

template <typename T, bool SHARED>
__global__ __launch_bounds__(64) void mv_solve_kernel(const MvSolve a) {
  const long q = (long)blockIdx.x * 64 + threadIdx.x;
  if (q >= a.n) return;
  const long g = q / a.group_div;
  const double* cams = SHARED ? a.cams : a.cams + g * (long)a.S * 12;
  const T* tp = static_cast<const T*>(a.tracks) + g * a.track_stride_q;
  const long wrow = a.weight_rows ? (long)a.weight_rows[q] : q;
  const uint8_t* w8 = static_cast<const uint8_t*>(a.weights) + (a.weight_kind == 1 ? wrow * a.weight_stride_row : 0);
  const double* w64 = static_cast<const double*>(a.weights) + (a.weight_kind == 2 ? wrow * a.weight_stride_row : 0);
  double m[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) m[k] = 0.0;
  int used = 0;
#pragma unroll 2
  for (int s = 0; s < a.S; ++s) {
    const typename Vec2<T>::type uv = *reinterpret_cast<const typename Vec2<T>::type*>(tp + (long)s * a.track_stride_s);
    double w = 1.0;
    if (a.weight_kind == 1) w = w8[(long)s * a.weight_stride_s] ? 1.0 : 0.0;
    else if (a.weight_kind == 2) w = w64[(long)s * a.weight_stride_s];
    double u = (double)uv.x, v = (double)uv.y;
    if (w != 0.0) ++used;
    else if (a.zero_masked) { u = 0.0; v = 0.0; }
    const double* P = cams + 12 * s;
    const double nr = sqrt(u * u + v * v + 1.0);
    const double r0 = u / nr, r1 = v / nr, r2 = 1.0 / nr;
    double t[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double rp = r0 * P[k] + r1 * P[4 + k] + r2 * P[8 + k];
      t[k] = (P[k] - r0 * rp) * w; t[4 + k] = (P[4 + k] - r1 * rp) * w; t[8 + k] = (P[8 + k] - r2 * rp) * w;
    }
    int e = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = i; j < 4; ++j) { m[e] += t[i] * t[j] + t[4 + i] * t[4 + j] + t[8 + i] * t[8 + j]; ++e; }
  }
  double X0, X1, X2;
  bool invalid;
  if (used < 2) {                               // no defined answer (the reference: an arbitrary null vector)
    X0 = X1 = X2 = __builtin_nan("");
    invalid = true;
  } else {
    double v[4];
    smallest_eigvec4<kMvSweeps4>(m, kMvTol4, v);
    X0 = v[0] / v[3]; X1 = v[1] / v[3]; X2 = v[2] / v[3];
    invalid = false;
    if (a.out_invalid) {
      for (int s = 0; s < a.S; ++s) {
        const double* P = cams + 12 * s;
        const double z = P[8] * X0 + P[9] * X1 + P[10] * X2 + P[11];
        invalid = invalid || (z <= 0.0);
      }
    }
  }
  a.out_points[3 * q] = X0; a.out_points[3 * q + 1] = X1; a.out_points[3 * q + 2] = X2;
  if (a.out_invalid) a.out_invalid[q] = invalid ? 1 : 0;
}

// projection centres -R^T t
__global__ __launch_bounds__(256) void mv_centers_kernel(const double* __restrict__ cams, long count,
                                                         double* __restrict__ centers) {
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  if (s >= count) return;
  camera_centre(cams + 12 * s, centers + 3 * s);
}

// per point: the largest angle over all camera pairs (FLAG_ONLY: whether some pair reaches `thr`, scan stops wave-wide once
// every lane has its answer).  A non-finite point: angle 0, flag 0.
template <bool SHARED, bool FLAG_ONLY>
__global__ __launch_bounds__(64) void mv_max_angle_kernel(const double* __restrict__ centers, const double* __restrict__ points,
                                                          long n, int S, int group_div, double thr,
                                                          double* __restrict__ out_angle, uint8_t* __restrict__ out_flag) {
  const long q = (long)blockIdx.x * 64 + threadIdx.x;
  const bool in = q < n;
  const long qq = in ? q : n - 1;                       // (lanes past the end follow lane n-1: the loops stay wave-uniform)
  const double* c = SHARED ? centers : centers + (qq / group_div) * (long)S * 3;
  const double X0 = points[3 * qq], X1 = points[3 * qq + 1], X2 = points[3 * qq + 2];
  const double big = 1.7976931348623157e308;
  const bool live = in && (fabs(X0) <= big) && (fabs(X1) <= big) && (fabs(X2) <= big);
  double best = 0.0;
  bool found = live && (0.0 >= thr);                     // (the diagonal pairs: angle 0)
  if (FLAG_ONLY ? !__all(found || !live) : __any(live)) {
    for (int i = 0; i + 1 < S; ++i) {
      const double a0 = c[3 * i], a1 = c[3 * i + 1], a2 = c[3 * i + 2];
      const double r1 = sqnorm3(X0 - a0, X1 - a1, X2 - a2);
      for (int j = i + 1; j < S; ++j) {
        const double b0 = c[3 * j], b1 = c[3 * j + 1], b2 = c[3 * j + 2];
        const double bsq = sqnorm3(a0 - b0, a1 - b1, a2 - b2);
        const double r2 = sqnorm3(X0 - b0, X1 - b1, X2 - b2);
        if (FLAG_ONLY) {
          if (live && !found && mv_angle_deg(r1, r2, bsq, kMvEps) >= thr) found = true;
        } else if (live) {
          best = fmax(best, mv_angle_deg(r1, r2, bsq, kMvEps));
        }
      }
      if (FLAG_ONLY && __all(found || !live)) break;
    }
  }
  if (!in) return;
  if (!FLAG_ONLY) {
    out_angle[q] = best;
    found = live && (best >= thr);
  }
  if (out_flag) out_flag[q] = found ? 1 : 0;
}

// (B, S*S) table: one thread per entry, the pair index fastest (coalesced stores)
template <bool SHARED>
__global__ __launch_bounds__(256) void mv_angle_table_kernel(const double* __restrict__ centers, const double* __restrict__ points,
                                                             long B, int S, double eps, double* __restrict__ out) {
  const long SS = (long)S * S;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * SS) return;
  const long b = idx / SS;
  const int k = (int)(idx - b * SS), i = k / S, j = k - i * S;
  const double* c = SHARED ? centers : centers + b * (long)S * 3;
  const double X0 = points[3 * b], X1 = points[3 * b + 1], X2 = points[3 * b + 2];
  const double a0 = c[3 * i], a1 = c[3 * i + 1], a2 = c[3 * i + 2], b0 = c[3 * j], b1 = c[3 * j + 1], b2 = c[3 * j + 2];
  out[idx] = mv_angle_deg(sqnorm3(X0 - a0, X1 - a1, X2 - a2), sqnorm3(X0 - b0, X1 - b1, X2 - b2),
                          sqnorm3(a0 - b0, a1 - b1, a2 - b2), eps);
}

// (K, P) table of given centre pairs: the point index fastest
__global__ __launch_bounds__(256) void mv_angle_pairs_kernel(const double* __restrict__ c1, const double* __restrict__ c2, long K,
                                                             const double* __restrict__ points, long P, double eps,
                                                             double* __restrict__ out) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= K * P) return;
  const long k = idx / P, p = idx - k * P;
  const double X0 = points[3 * p], X1 = points[3 * p + 1], X2 = points[3 * p + 2];
  const double a0 = c1[3 * k], a1 = c1[3 * k + 1], a2 = c1[3 * k + 2], b0 = c2[3 * k], b1 = c2[3 * k + 1], b2 = c2[3 * k + 2];
  out[idx] = mv_angle_deg(sqnorm3(X0 - a0, X1 - a1, X2 - a2), sqnorm3(X0 - b0, X1 - b1, X2 - b2),
                          sqnorm3(a0 - b0, a1 - b1, a2 - b2), eps);
}

// calculate_normalized_angular_error_batched: out (P,B,N), the observation index fastest
__global__ __launch_bounds__(256) void mv_angular_error_kernel(const double* __restrict__ p2, const double* __restrict__ p3,
                                                               const double* __restrict__ cams, long B, long N, long P,
                                                               int to_degree, double* __restrict__ out_angle,
                                                               double* __restrict__ out_cos) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= P * B * N) return;
  const long p = idx / (B * N), r = idx - p * (B * N), b = r / N, nn = r - b * N;
  const double u = p2[2 * (b * N + nn)], v = p2[2 * (b * N + nn) + 1];
  const double* X = p3 + 3 * (p * N + nn);
  const double* C = cams + 12 * b;
  const double y0 = C[0] * X[0] + C[1] * X[1] + C[2] * X[2] + C[3];
  const double y1 = C[4] * X[0] + C[5] * X[1] + C[6] * X[2] + C[7];
  const double y2 = C[8] * X[0] + C[9] * X[1] + C[10] * X[2] + C[11];
  const double n1 = fmax(sqrt(u * u + v * v + 1.0), 1e-12);          // F.normalize: x / max(|x|, 1e-12)
  const double n2 = fmax(sqrt(y0 * y0 + y1 * y1 + y2 * y2), 1e-12);
  double c = (u / n1) * (y0 / n2) + (v / n1) * (y1 / n2) + (1.0 / n1) * (y2 / n2);
  c = (c != c) ? c : fmin(fmax(c, -1.0), 1.0);
  double th = acos(c);
  if (to_degree) th = th * (180.0 / kMvPi);
  out_angle[idx] = th;
  out_cos[idx] = c;
}

int launch_centers(const double* cams, long count, double* out, hipStream_t st) {
  if (count <= 0) return VGG_OK;
  hipLaunchKernelGGL(mv_centers_kernel, dim3(div_up(count, 256)), dim3(256), 0, st, cams, count, out);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int launch_max_angle(const double* centers, bool shared, int group_div, const double* points, long n, int S, int angle_mode,
                     double thr, double* out_angle, uint8_t* out_flag, hipStream_t st) {
  const dim3 grid(div_up(n, 64)), block(64);
  if (angle_mode == 2) {
    if (shared) hipLaunchKernelGGL((mv_max_angle_kernel<true, true>), grid, block, 0, st, centers, points, n, S, group_div, thr, out_angle, out_flag);
    else hipLaunchKernelGGL((mv_max_angle_kernel<false, true>), grid, block, 0, st, centers, points, n, S, group_div, thr, out_angle, out_flag);
  } else {
    if (shared) hipLaunchKernelGGL((mv_max_angle_kernel<true, false>), grid, block, 0, st, centers, points, n, S, group_div, thr, out_angle, out_flag);
    else hipLaunchKernelGGL((mv_max_angle_kernel<false, false>), grid, block, 0, st, centers, points, n, S, group_div, thr, out_angle, out_flag);
  }
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

bool angle_args_ok(int angle_mode, const double* out_angle, const uint8_t* out_flag, const void* workspace) {
  if (angle_mode == 1) return out_angle != nullptr && workspace != nullptr;
  if (angle_mode == 2) return out_flag != nullptr && workspace != nullptr;
  return angle_mode == 0;
}

constexpr long kMaxBlocks = 2147483647L;      // gridDim.x (and, for the one-lane-per-point kernels, a bound on n)

}  // namespace
}  // namespace vgg

using namespace vgg;

extern "C" {

size_t vggx_multiview_workspace_bytes(long cam_groups, int S) {
  if (cam_groups < 1 || S < 1) return 0;
  return sizeof(double) * 3 * (size_t)cam_groups * (size_t)S;
}

int vggx_view_centers(const double* cams, long count, double* out_centers, void* stream) {
  if (count < 0 || (count > 0 && (!cams || !out_centers))) return VGG_ERR_INVALID_ARGUMENT;
  return launch_centers(cams, count, out_centers, (hipStream_t)stream);
}

int vggx_multiview_triangulate(const double* cams, long cam_groups, int group_div, const void* tracks, int tracks_are_f64,
                               long track_stride_q, long track_stride_s, const void* weights, int weight_kind,
                               long weight_stride_row, long weight_stride_s, const int64_t* weight_rows, long n, int S,
                               int zero_masked, int angle_mode, double min_tri_angle, double* out_points,
                               uint8_t* out_invalid_cheirality, double* out_max_angle, uint8_t* out_angle_flag,
                               void* workspace, void* stream) {
  if (n < 0 || S < 1 || cam_groups < 1 || group_div < 1 || weight_kind < 0 || weight_kind > 2 ||
      !angle_args_ok(angle_mode, out_max_angle, out_angle_flag, workspace))
    return VGG_ERR_INVALID_ARGUMENT;
  if (n == 0) return VGG_OK;
  if (!cams || !tracks || !out_points || (weight_kind != 0 && !weights) || (weight_kind == 0 && weight_rows) ||
      track_stride_q < 0 || track_stride_s < 0 || weight_stride_row < 0 || weight_stride_s < 0 ||
      (track_stride_q & 1) || (track_stride_s & 1) || ((uintptr_t)tracks % (tracks_are_f64 ? 16 : 8)) != 0 ||
      (cam_groups > 1 && (n - 1) / group_div >= cam_groups) || n > kMaxBlocks)
    return VGG_ERR_INVALID_ARGUMENT;
  hipStream_t st = (hipStream_t)stream;
  const bool shared = cam_groups == 1;
  MvSolve a;
  a.cams = cams; a.tracks = tracks; a.weights = weights; a.weight_rows = weight_rows;
  a.track_stride_q = track_stride_q; a.track_stride_s = track_stride_s;
  a.weight_stride_row = weight_stride_row; a.weight_stride_s = weight_stride_s; a.n = n;
  a.group_div = group_div; a.weight_kind = weight_kind; a.S = S; a.zero_masked = zero_masked ? 1 : 0;
  a.out_points = out_points; a.out_invalid = out_invalid_cheirality;
  const dim3 grid(div_up(n, 64)), block(64);
  if (tracks_are_f64) {
    if (shared) hipLaunchKernelGGL((mv_solve_kernel<double, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((mv_solve_kernel<double, false>), grid, block, 0, st, a);
  } else {
    if (shared) hipLaunchKernelGGL((mv_solve_kernel<float, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((mv_solve_kernel<float, false>), grid, block, 0, st, a);
  }
  VGG_LAUNCH_CHECK();
  if (angle_mode == 0) return VGG_OK;
  double* centers = static_cast<double*>(workspace);
  const int rc = launch_centers(cams, cam_groups * (long)S, centers, st);
  if (rc != VGG_OK) return rc;
  return launch_max_angle(centers, shared, group_div, out_points, n, S, angle_mode, min_tri_angle, out_max_angle,
                          out_angle_flag, st);
}

int vggx_max_tri_angle(const double* cams, long cam_groups, int group_div, const double* points, long n, int S,
                       int angle_mode, double min_tri_angle, double* out_max_angle, uint8_t* out_angle_flag,
                       void* workspace, void* stream) {
  if (n < 0 || S < 1 || cam_groups < 1 || group_div < 1 || angle_mode == 0 ||
      !angle_args_ok(angle_mode, out_max_angle, out_angle_flag, workspace))
    return VGG_ERR_INVALID_ARGUMENT;
  if (n == 0) return VGG_OK;
  if (!cams || !points || (cam_groups > 1 && (n - 1) / group_div >= cam_groups) || n > kMaxBlocks)
    return VGG_ERR_INVALID_ARGUMENT;
  hipStream_t st = (hipStream_t)stream;
  double* centers = static_cast<double*>(workspace);
  const int rc = launch_centers(cams, cam_groups * (long)S, centers, st);
  if (rc != VGG_OK) return rc;
  return launch_max_angle(centers, cam_groups == 1, group_div, points, n, S, angle_mode, min_tri_angle, out_max_angle,
                          out_angle_flag, st);
}

int vggx_tri_angle_table(const double* cams, long cam_groups, const double* points, long B, int S, double eps, double* out,
                         void* workspace, void* stream) {
  if (B < 0 || S < 1 || (cam_groups != 1 && cam_groups != B)) return VGG_ERR_INVALID_ARGUMENT;
  if (B == 0) return VGG_OK;
  if (!cams || !points || !out || !workspace) return VGG_ERR_INVALID_ARGUMENT;
  const long total = B * (long)S * S;
  if ((total + 255) / 256 > kMaxBlocks) return VGG_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  double* centers = static_cast<double*>(workspace);
  const int rc = launch_centers(cams, cam_groups * (long)S, centers, st);
  if (rc != VGG_OK) return rc;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  if (cam_groups == 1 && B != 1) hipLaunchKernelGGL((mv_angle_table_kernel<true>), grid, block, 0, st, centers, points, B, S, eps, out);
  else hipLaunchKernelGGL((mv_angle_table_kernel<false>), grid, block, 0, st, centers, points, B, S, eps, out);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vggx_tri_angle_pairs(const double* center1, const double* center2, long K, const double* points, long P, double eps,
                         double* out, void* stream) {
  if (K < 0 || P < 0) return VGG_ERR_INVALID_ARGUMENT;
  if (K == 0 || P == 0) return VGG_OK;
  if (!center1 || !center2 || !points || !out) return VGG_ERR_INVALID_ARGUMENT;
  const long total = K * P;
  if ((total + 255) / 256 > kMaxBlocks) return VGG_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(mv_angle_pairs_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, center1,
                     center2, K, points, P, eps, out);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vggx_angular_error(const double* point2D, const double* point3D, const double* cams, long B, long N, long P,
                       int to_degree, double* out_angle, double* out_cos, void* stream) {
  if (B < 0 || N < 0 || P < 0) return VGG_ERR_INVALID_ARGUMENT;
  if (B == 0 || N == 0 || P == 0) return VGG_OK;
  if (!point2D || !point3D || !cams || !out_angle || !out_cos) return VGG_ERR_INVALID_ARGUMENT;
  const long total = P * B * N;
  if ((total + 255) / 256 > kMaxBlocks) return VGG_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(mv_angular_error_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     point2D, point3D, cams, B, N, P, to_degree, out_angle, out_cos);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

}  // extern "C"
