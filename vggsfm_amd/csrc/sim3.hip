// Sim(3) alignment of 3D-3D correspondences (weighted Umeyama, hypothesis scoring, 3-point LO-RANSAC) and the all-pairs
// pose errors of vggsfm/utils/metric.py.  DESIGN.md section 20.
//
// float64, no FMA contraction (-ffp-contract=off), no floating-point atomics, every sum in a fixed order.
//   fit     N <= kFitSingle: one workgroup of 256 threads per problem (means, block tree, centred moments, block tree,
//           thread 0 finishes).  Larger N: G <= 256 workgroups per problem write the partial sums of the means, G workgroups
//           add those partials (one per thread, the same block tree) and write the partial centred moments, one workgroup
//           per problem adds them the same way and finishes.  G depends on N alone, so a problem's result does not depend on what else is in the launch
//   score   a workgroup holds a tile of kTile hypotheses in LDS and one part of the points (kPts per thread) in registers:
//           the points are read once per tile, the hypotheses walk past them; per hypothesis a wavefront butterfly, the
//           four wavefronts in their order, one partial per (hypothesis, part) into the workspace; a second kernel adds
//           the parts in their order
//   ransac  minimal fits (one thread per sample), score, select (one workgroup per problem, a total order), then the LO
//           rounds as launches that turn into no-ops on the device once a problem has stopped: nothing returns to the host
//   pairs   one thread per camera pair; the two relative poses live in registers
// A masked-out point (mask or weight 0) is skipped: nothing read from its slots enters a result.
#include "common.hpp"
#include "jacobi.hpp"
#include "kabsch3.hpp"
#include "mvs/mvs_geometry.hpp"
#include "support.hpp"
#include "../../include/vggsfm_amd_sim3.h"

namespace vgg {

constexpr int kFitSingle = 4096;     // the largest N that one workgroup fits alone
constexpr int kFitPart = 1024;       // points per workgroup of the multi-workgroup fit ...
constexpr int kFitMaxParts = 256;    // ... until this many workgroups per problem
constexpr int kTile = 32;            // hypotheses per workgroup of the score pass
constexpr int kPts = 8;              // points per thread of the score pass, in registers
constexpr int kScorePart = 256 * kPts;  // points per workgroup of the score pass
constexpr int kMaxGridYZ = 65535;
static_assert(kFitMaxParts <= 256, "ordered_partials holds one partial per thread of a workgroup");
constexpr int kSweepsScatter = 10;   // Jacobi sweeps of the 3x3 source scatter (sym3_eigenvalues)
constexpr double kCollinear = 1e-12; // second / first eigenvalue of the source scatter at or below which a set is collinear
constexpr double kAngleEps = 1e-15;  // the reference's clamp (metric.py rotation_angle, compare_translation_by_angle)
constexpr double kDegrees = 57.295779513082320876798154814105;

struct Sim3Layout {
  int G, P;
  size_t hyp, hvalid, counts, sums, pc, ps, fit1, fit2, cand_T, cand_valid, cand_count, cand_sum, active, changed, acc_now, total;
};

inline int fit_parts(int N) { return N <= kFitSingle ? 1 : (div_up(N, kFitPart) < kFitMaxParts ? div_up(N, kFitPart) : kFitMaxParts); }
inline int score_parts(int N) { const int p = div_up(N, kScorePart); return p < 1 ? 1 : p; }

inline Sim3Layout sim3_layout(int B, int N, int H) {
  Sim3Layout L;
  L.G = fit_parts(N); L.P = score_parts(N);
  const size_t b = (size_t)B, h = (size_t)(H < 1 ? 1 : H);
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) / 256 * 256; return o; };
  L.hyp = take(b * h * 13 * 8); L.hvalid = take(b * h); L.counts = take(b * h * 4); L.sums = take(b * h * 8);
  L.pc = take(b * h * L.P * 4); L.ps = take(b * h * L.P * 8);
  L.fit1 = take(b * L.G * 8 * 8); L.fit2 = take(b * L.G * 16 * 8);
  L.cand_T = take(b * 13 * 8); L.cand_valid = take(b); L.cand_count = take(b * 4); L.cand_sum = take(b * 8);
  L.active = take(b * 4); L.changed = take(b * 4); L.acc_now = take(b * 4);
  L.total = at;
  return L;
}

__device__ __forceinline__ void identity13(double* T) {
  T[0] = 1.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) T[1 + k] = (k % 4 == 0) ? 1.0 : 0.0;
  T[10] = 0.0; T[11] = 0.0; T[12] = 0.0;
}

// weight of point i: doubles, a mask, or 1; anything that is not > 0 (NaN included) is 0
__device__ __forceinline__ double weight_of(const double* wd, const uint8_t* wm, size_t i) {
  if (wd) { const double w = wd[i]; return (w > 0.0) ? w : 0.0; }
  if (wm) return wm[i] ? 1.0 : 0.0;
  return 1.0;
}

// v[0] = W, v[1] = number of points of positive weight, v[2..4] = sum w src, v[5..7] = sum w tgt
__device__ __forceinline__ void add_mean_terms(const double* s, const double* t, double w, double* v) {
  v[0] = v[0] + w; v[1] = v[1] + 1.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) { v[2 + c] = v[2 + c] + w * s[c]; v[5 + c] = v[5 + c] + w * t[c]; }
}
// mu[0..2] = mean of src, mu[3..5] = mean of tgt (0 when nothing carries weight: no NaN reaches the second pass)
__device__ __forceinline__ void means_of(const double* v, double* mu) {
  const bool ok = v[0] > 0.0;
#pragma unroll
  for (int c = 0; c < 6; ++c) mu[c] = ok ? v[2 + c] / v[0] : 0.0;
}
// q[3 r + c] = sum w dt_r ds_c; q[9..14] = sum w ds ds^T (xx, xy, xz, yy, yz, zz)
__device__ __forceinline__ void add_moment_terms(const double* s, const double* t, double w, const double* mu, double* q) {
  double ds[3], dt[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) { ds[c] = s[c] - mu[c]; dt[c] = t[c] - mu[3 + c]; }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) q[3 * r + c] = q[3 * r + c] + (w * dt[r]) * ds[c];
  q[9] = q[9] + (w * ds[0]) * ds[0]; q[10] = q[10] + (w * ds[0]) * ds[1]; q[11] = q[11] + (w * ds[0]) * ds[2];
  q[12] = q[12] + (w * ds[1]) * ds[1]; q[13] = q[13] + (w * ds[1]) * ds[2]; q[14] = q[14] + (w * ds[2]) * ds[2];
}

// eigenvalues of the symmetric 3x3 matrix (xx, xy, xz, yy, yz, zz) by cyclic Jacobi, in descending order
__device__ inline void sym3_eigenvalues(const double* S, double* ev) {
  double A[3][3] = {{S[0], S[1], S[2]}, {S[1], S[3], S[4]}, {S[2], S[4], S[5]}};
  jacobi_sym3<kSweepsScatter, false>(A, nullptr);
  const double a = A[0][0], b = A[1][1], c = A[2][2];
  ev[0] = fmax(a, fmax(b, c));
  ev[2] = fmin(a, fmin(b, c));
  ev[1] = ((a + b) + c) - (ev[0] + ev[2]);
  ev[1] = fmin(ev[0], fmax(ev[2], ev[1]));
}

// the transform from the sums of the two passes; false (and the identity) for a set that determines none
__device__ inline bool sim3_finish(const double* v, const double* mu, const double* q, int estimate_scale, double* T) {
  identity13(T);
  const double W = v[0];
  if (!(v[1] >= 3.0) || !(W > 0.0)) return false;
  double Sig[9], Sc[6];
#pragma unroll
  for (int k = 0; k < 9; ++k) Sig[k] = q[k] / W;
#pragma unroll
  for (int k = 0; k < 6; ++k) Sc[k] = q[9 + k] / W;
  const double var = (Sc[0] + Sc[3]) + Sc[5];
  if (!(var > 0.0)) return false;
  double ev[3];
  sym3_eigenvalues(Sc, ev);
  if (!(ev[1] > kCollinear * ev[0])) return false;
  double R[9];
  const double tr = kabsch3(Sig, R);
  const double s = estimate_scale ? tr / var : 1.0;
  double t[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) t[r] = mu[3 + r] - s * ((R[3 * r] * mu[0] + R[3 * r + 1] * mu[1]) + R[3 * r + 2] * mu[2]);
  bool fin = isfinite(s) && s > 0.0 && isfinite(t[0]) && isfinite(t[1]) && isfinite(t[2]);
#pragma unroll
  for (int k = 0; k < 9; ++k) fin = fin && isfinite(R[k]);
  if (!fin) return false;
  T[0] = s;
#pragma unroll
  for (int k = 0; k < 9; ++k) T[1 + k] = R[k];
  T[10] = t[0]; T[11] = t[1]; T[12] = t[2];
  return true;
}

// squared residual of one correspondence under T
__device__ __forceinline__ double sim3_residual_sq(const double* T, const double* s, const double* t) {
  double e = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double y = (T[1 + 3 * r] * s[0] + T[2 + 3 * r] * s[1]) + T[3 + 3 * r] * s[2];
    const double d = t[r] - (T[0] * y + T[10 + r]);
    e = e + d * d;
  }
  return e;
}

// a problem of the LO rounds that has stopped (or never started) is skipped by every kernel of the round
__device__ __forceinline__ bool lo_runs(const int32_t* active, const int32_t* changed, int b) {
  return !active || (active[b] != 0 && changed[b] != 0);
}

// ------------------------------------------------------------------------------------------------------------- fit
__global__ __launch_bounds__(256) void sim3_fit_single_kernel(const double* __restrict__ src, const double* __restrict__ tgt,
                                                              const double* __restrict__ wd, const uint8_t* __restrict__ wm, int N,
                                                              int estimate_scale, double* __restrict__ out_T,
                                                              uint8_t* __restrict__ out_valid, const int32_t* __restrict__ active,
                                                              const int32_t* __restrict__ changed) {
  __shared__ double red[15][256];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (!lo_runs(active, changed, b)) return;
  const size_t base = (size_t)b * N;
  double v[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tot[8], mu[6];
  for (int i = tid; i < N; i += 256) {
    const double w = weight_of(wd, wm, base + i);
    if (w > 0.0) add_mean_terms(src + (base + i) * 3, tgt + (base + i) * 3, w, v);
  }
  block_tree_sum<8>(red, v, tot);
  means_of(tot, mu);
  double q[15], qt[15];
#pragma unroll
  for (int k = 0; k < 15; ++k) q[k] = 0.0;
  for (int i = tid; i < N; i += 256) {
    const double w = weight_of(wd, wm, base + i);
    if (w > 0.0) add_moment_terms(src + (base + i) * 3, tgt + (base + i) * 3, w, mu, q);
  }
  block_tree_sum<15>(red, q, qt);
  if (tid == 0) {
    double T[13];
    const bool ok = sim3_finish(tot, mu, qt, estimate_scale, T);
#pragma unroll
    for (int k = 0; k < 13; ++k) out_T[(size_t)b * 13 + k] = T[k];
    out_valid[b] = ok ? 1 : 0;
  }
}

// the G <= 256 partials of Q quantities (part[g * stride + q]) added by the fixed halving tree, one partial per thread;
// every thread gets the sums
template <int Q>
__device__ __forceinline__ void ordered_partials(double (*red)[256], const double* part, int G, int stride, double* out) {
  double v[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) v[q] = ((int)threadIdx.x < G) ? part[(size_t)threadIdx.x * stride + q] : 0.0;
  block_tree_sum<Q>(red, v, out);
}

__global__ __launch_bounds__(256) void sim3_fit_means_kernel(const double* __restrict__ src, const double* __restrict__ tgt,
                                                             const double* __restrict__ wd, const uint8_t* __restrict__ wm, int N,
                                                             int G, double* __restrict__ fit1, const int32_t* __restrict__ active,
                                                             const int32_t* __restrict__ changed) {
  __shared__ double red[8][256];
  const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  if (!lo_runs(active, changed, b)) return;
  const int len = (N + G - 1) / G, lo = g * len, hi = (lo + len < N) ? lo + len : N;
  const size_t base = (size_t)b * N;
  double v[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tot[8];
  for (int i = lo + tid; i < hi; i += 256) {
    const double w = weight_of(wd, wm, base + i);
    if (w > 0.0) add_mean_terms(src + (base + i) * 3, tgt + (base + i) * 3, w, v);
  }
  block_tree_sum<8>(red, v, tot);
  if (tid < 8) fit1[((size_t)b * G + g) * 8 + tid] = tot[tid];
}

__global__ __launch_bounds__(256) void sim3_fit_moments_kernel(const double* __restrict__ src, const double* __restrict__ tgt,
                                                               const double* __restrict__ wd, const uint8_t* __restrict__ wm, int N,
                                                               int G, const double* __restrict__ fit1, double* __restrict__ fit2,
                                                               const int32_t* __restrict__ active, const int32_t* __restrict__ changed) {
  __shared__ double red[15][256];
  const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  if (!lo_runs(active, changed, b)) return;
  double tot[8], mu[6];
  ordered_partials<8>(red, fit1 + (size_t)b * G * 8, G, 8, tot);
  means_of(tot, mu);
  const int len = (N + G - 1) / G, lo = g * len, hi = (lo + len < N) ? lo + len : N;
  const size_t base = (size_t)b * N;
  double q[15], qt[15];
#pragma unroll
  for (int k = 0; k < 15; ++k) q[k] = 0.0;
  for (int i = lo + tid; i < hi; i += 256) {
    const double w = weight_of(wd, wm, base + i);
    if (w > 0.0) add_moment_terms(src + (base + i) * 3, tgt + (base + i) * 3, w, mu, q);
  }
  block_tree_sum<15>(red, q, qt);
  if (tid < 15) fit2[((size_t)b * G + g) * 16 + tid] = qt[tid];
}

__global__ __launch_bounds__(256) void sim3_fit_final_kernel(int G, int estimate_scale, const double* __restrict__ fit1,
                                                             const double* __restrict__ fit2, double* __restrict__ out_T,
                                                             uint8_t* __restrict__ out_valid, const int32_t* __restrict__ active,
                                                             const int32_t* __restrict__ changed) {
  __shared__ double red[15][256];
  const int b = blockIdx.x;
  if (!lo_runs(active, changed, b)) return;
  double tot[8], mu[6], qt[15];
  ordered_partials<8>(red, fit1 + (size_t)b * G * 8, G, 8, tot);
  means_of(tot, mu);
  ordered_partials<15>(red, fit2 + (size_t)b * G * 16, G, 16, qt);
  if (threadIdx.x == 0) {
    double T[13];
    const bool ok = sim3_finish(tot, mu, qt, estimate_scale, T);
    for (int k = 0; k < 13; ++k) out_T[(size_t)b * 13 + k] = T[k];
    out_valid[b] = ok ? 1 : 0;
  }
}

// the 3-point hypotheses: one thread per sample
__global__ __launch_bounds__(64) void sim3_minimal_kernel(const double* __restrict__ src, const double* __restrict__ tgt,
                                                          const uint8_t* __restrict__ mask, const int32_t* __restrict__ samples, int N,
                                                          int H, int estimate_scale, double* __restrict__ hyp,
                                                          uint8_t* __restrict__ hvalid) {
  const int h = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (h >= H) return;
  const size_t slot = (size_t)b * H + h, base = (size_t)b * N;
  const int32_t i0 = samples[slot * 3], i1 = samples[slot * 3 + 1], i2 = samples[slot * 3 + 2];
  bool ok = i0 >= 0 && i1 >= 0 && i2 >= 0 && i0 < N && i1 < N && i2 < N && i0 != i1 && i0 != i2 && i1 != i2;
  if (ok && mask) ok = mask[base + i0] && mask[base + i1] && mask[base + i2];
  double T[13];
  identity13(T);
  if (ok) {
    const int32_t idx[3] = {i0, i1, i2};
    double v[8] = {0, 0, 0, 0, 0, 0, 0, 0}, mu[6], q[15];
#pragma unroll
    for (int k = 0; k < 3; ++k) add_mean_terms(src + (base + idx[k]) * 3, tgt + (base + idx[k]) * 3, 1.0, v);
    means_of(v, mu);
#pragma unroll
    for (int k = 0; k < 15; ++k) q[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) add_moment_terms(src + (base + idx[k]) * 3, tgt + (base + idx[k]) * 3, 1.0, mu, q);
    ok = sim3_finish(v, mu, q, estimate_scale, T);
  }
  for (int k = 0; k < 13; ++k) hyp[slot * 13 + k] = T[k];
  hvalid[slot] = ok ? 1 : 0;
}

// ----------------------------------------------------------------------------------------------------------- score
// grid (P, tiles, B).  Partials [(b H + h) P + p]; a hypothesis that is invalid (or beyond H) costs nothing.
__global__ __launch_bounds__(256) void sim3_score_kernel(const double* __restrict__ src, const double* __restrict__ tgt,
                                                         const uint8_t* __restrict__ mask, const double* __restrict__ transforms,
                                                         const uint8_t* __restrict__ valid, const double* __restrict__ max_error, int N,
                                                         int H, int P, int32_t* __restrict__ pc, double* __restrict__ ps,
                                                         const int32_t* __restrict__ active, const int32_t* __restrict__ changed) {
  __shared__ double Ts[kTile][13];
  __shared__ int ok[kTile];
  __shared__ double wsum[4][kTile];
  __shared__ int wcnt[4][kTile];
  const int p = blockIdx.x, h0 = blockIdx.y * kTile, b = blockIdx.z, tid = threadIdx.x;
  if (!lo_runs(active, changed, b)) return;
  for (int k = tid; k < kTile * 13; k += 256) {
    const int j = k / 13, c = k - 13 * j;
    Ts[j][c] = (h0 + j < H) ? transforms[((size_t)b * H + h0 + j) * 13 + c] : 0.0;
  }
  if (tid < kTile) ok[tid] = (h0 + tid < H) ? (valid[(size_t)b * H + h0 + tid] != 0) : 0;
  __syncthreads();
  const double e = max_error[b], thr = e * e;
  const int len = (N + P - 1) / P, lo = p * len, hi = (lo + len < N) ? lo + len : N;      // len <= kScorePart = 256 kPts
  const size_t base = (size_t)b * N;
  // this thread's points of the part, in registers for the whole tile (a point that is masked out or beyond the part is
  // not read and counts for nothing)
  double s[kPts][3], t[kPts][3];
  bool have[kPts];
#pragma unroll
  for (int k = 0; k < kPts; ++k) {
    const int i = lo + tid + 256 * k;
    have[k] = i < hi && (!mask || mask[base + i]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      s[k][c] = have[k] ? src[(base + i) * 3 + c] : 0.0;
      t[k][c] = have[k] ? tgt[(base + i) * 3 + c] : 0.0;
    }
  }
  const int wave = tid >> 6;
#pragma unroll 2
  for (int j = 0; j < kTile; ++j) {
    int cnt = 0;
    double sum = 0.0;
    if (ok[j]) {                                         // (uniform)
      double T[13];
#pragma unroll
      for (int c = 0; c < 13; ++c) T[c] = Ts[j][c];
#pragma unroll
      for (int k = 0; k < kPts; ++k) {
        const double r = sim3_residual_sq(T, s[k], t[k]);
        const bool in = have[k] && r <= thr;
        cnt += in ? 1 : 0;
        sum = sum + (in ? r : 0.0);
      }
      cnt = wave_sum_i(cnt);
      sum = wave_sum(sum);
    }
    if ((tid & 63) == 0) { wcnt[wave][j] = cnt; wsum[wave][j] = sum; }
  }
  __syncthreads();
  if (tid < kTile && h0 + tid < H) {
    const size_t at = ((size_t)b * H + h0 + tid) * P + p;
    pc[at] = (wcnt[0][tid] + wcnt[1][tid]) + (wcnt[2][tid] + wcnt[3][tid]);
    ps[at] = ((wsum[0][tid] + wsum[1][tid]) + wsum[2][tid]) + wsum[3][tid];
  }
}

__global__ __launch_bounds__(256) void sim3_score_reduce_kernel(const uint8_t* __restrict__ valid, int H, int P, long total,
                                                                const int32_t* __restrict__ pc, const double* __restrict__ ps,
                                                                int32_t* __restrict__ counts, double* __restrict__ sums,
                                                                const int32_t* __restrict__ active, const int32_t* __restrict__ changed) {
  const long at = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (at >= total) return;
  if (!lo_runs(active, changed, (int)(at / H))) return;
  if (!valid[at]) { counts[at] = -1; sums[at] = 0.0; return; }
  int c = 0;
  double a = 0.0;
  for (int p = 0; p < P; ++p) { c += pc[(size_t)at * P + p]; a = a + ps[(size_t)at * P + p]; }
  counts[at] = c; sums[at] = a;
}

// ---------------------------------------------------------------------------------------------------------- ransac
__global__ __launch_bounds__(256) void sim3_select_kernel(int H, const double* __restrict__ hyp, const int32_t* __restrict__ counts,
                                                          const double* __restrict__ sums, double* __restrict__ out_T,
                                                          int32_t* __restrict__ out_num, double* __restrict__ out_sum,
                                                          int32_t* __restrict__ out_best, int32_t* __restrict__ out_lo,
                                                          int32_t* __restrict__ active, int32_t* __restrict__ changed,
                                                          int32_t* __restrict__ acc_now) {
  __shared__ int bc[256], bi[256];
  __shared__ double bs[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  int c = -1, idx = 2147483647;
  double s = 0.0;
  for (int h = tid; h < H; h += 256) {
    const int ch = counts[(size_t)b * H + h];
    const double sh = sums[(size_t)b * H + h];
    if (ch >= 0 && (c < 0 || ranks_before(ch, sh, h, c, s, idx))) { c = ch; s = sh; idx = h; }
  }
  bc[tid] = c; bs[tid] = s; bi[tid] = idx;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) {
      const int c2 = bc[tid + st], i2 = bi[tid + st];
      const double s2 = bs[tid + st];
      if (c2 >= 0 && (bc[tid] < 0 || ranks_before(c2, s2, i2, bc[tid], bs[tid], bi[tid]))) { bc[tid] = c2; bs[tid] = s2; bi[tid] = i2; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const bool found = bc[0] >= 0;
    double T[13];
    identity13(T);
    if (found) for (int k = 0; k < 13; ++k) T[k] = hyp[((size_t)b * H + bi[0]) * 13 + k];
    for (int k = 0; k < 13; ++k) out_T[(size_t)b * 13 + k] = T[k];
    out_num[b] = found ? bc[0] : 0;
    out_sum[b] = found ? bs[0] : 0.0;
    out_best[b] = found ? bi[0] : -1;
    out_lo[b] = 0;
    active[b] = found ? 1 : 0;
    changed[b] = 1;
    acc_now[b] = 0;
  }
}

// the inlier mask of the current transform.  first: written for every problem (zeros where nothing was found).
// Otherwise only where this round accepted a transform, and `changed` says whether any element differs from before
// (an integer OR: whatever the order, the value is the same)
__global__ __launch_bounds__(256) void sim3_mask_kernel(const double* __restrict__ src, const double* __restrict__ tgt,
                                                        const uint8_t* __restrict__ mask, const double* __restrict__ max_error, int N,
                                                        const double* __restrict__ cur_T, int first, const int32_t* __restrict__ active,
                                                        const int32_t* __restrict__ acc_now, int32_t* __restrict__ changed,
                                                        uint8_t* __restrict__ out_mask) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const size_t at = (size_t)b * N + i;
  if (first) {
    if (!active[b]) { out_mask[at] = 0; return; }
  } else if (!acc_now[b]) {
    return;
  }
  uint8_t in = 0;
  if (!mask || mask[at]) {
    double T[13];
#pragma unroll
    for (int k = 0; k < 13; ++k) T[k] = cur_T[(size_t)b * 13 + k];
    const double e = max_error[b];
    in = sim3_residual_sq(T, src + at * 3, tgt + at * 3) <= e * e ? 1 : 0;
  }
  if (!first && out_mask[at] != in) atomicOr(changed + b, 1);
  out_mask[at] = in;
}

__global__ __launch_bounds__(64) void sim3_lo_decide_kernel(int B, const double* __restrict__ cand_T, const uint8_t* __restrict__ cand_valid,
                                                            const int32_t* __restrict__ cand_count, const double* __restrict__ cand_sum,
                                                            double* __restrict__ out_T, int32_t* __restrict__ out_num,
                                                            double* __restrict__ out_sum, int32_t* __restrict__ out_lo,
                                                            int32_t* __restrict__ active, int32_t* __restrict__ changed,
                                                            int32_t* __restrict__ acc_now) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  if (!active[b] || !changed[b] || !cand_valid[b]) { active[b] = 0; acc_now[b] = 0; return; }
  const int c = cand_count[b];
  const double s = cand_sum[b];
  if (c > out_num[b] || (c == out_num[b] && s < out_sum[b])) {
    for (int k = 0; k < 13; ++k) out_T[(size_t)b * 13 + k] = cand_T[(size_t)b * 13 + k];
    out_num[b] = c; out_sum[b] = s; out_lo[b] = out_lo[b] + 1;
    acc_now[b] = 1; changed[b] = 0;
  } else {
    active[b] = 0; acc_now[b] = 0;
  }
}

// success, and what a failed problem reports; `active` is reused as the success flag the mask pass reads
__global__ __launch_bounds__(64) void sim3_final_kernel(int B, int min_inliers, double* __restrict__ out_T, int32_t* __restrict__ out_num,
                                                        double* __restrict__ out_sum, const int32_t* __restrict__ out_best,
                                                        uint8_t* __restrict__ out_success, int32_t* __restrict__ active) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const bool ok = out_best[b] >= 0 && out_num[b] >= min_inliers;
  if (!ok) {
    double T[13];
    identity13(T);
    for (int k = 0; k < 13; ++k) out_T[(size_t)b * 13 + k] = T[k];
    out_num[b] = 0; out_sum[b] = 0.0;
  }
  out_success[b] = ok ? 1 : 0;
  active[b] = ok ? 1 : 0;
}
__global__ __launch_bounds__(256) void sim3_clear_failed_kernel(int N, const int32_t* __restrict__ active, uint8_t* __restrict__ out_mask) {
  const int b = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N && !active[b]) out_mask[(size_t)b * N + i] = 0;
}

// ------------------------------------------------------------------------------------------------------ pair errors
// (relative_pose, [R|t] of view j from view i as 3 x 4: mvs/mvs_geometry.hpp)
__global__ __launch_bounds__(256) void pose_pair_errors_kernel(const double* __restrict__ pred, const double* __restrict__ gt, int S,
                                                               long pairs, double* __restrict__ out_rot, double* __restrict__ out_trans) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pairs) return;
  // row i of the strict upper triangle starts at i (2 S - i - 1) / 2
  const double m = 2.0 * S - 1.0;
  long i = (long)((m - sqrt(m * m - 8.0 * (double)p)) * 0.5);
  i = i < 0 ? 0 : (i > S - 2 ? S - 2 : i);
  while (i > 0 && i * (2L * S - i - 1) / 2 > p) --i;
  while (i < S - 2 && (i + 1) * (2L * S - i - 2) / 2 <= p) ++i;
  const long j = p - i * (2L * S - i - 1) / 2 + i + 1;
  double Pi[12], Pj[12], Tg[12], Tp[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) { Pi[k] = gt[i * 12 + k]; Pj[k] = gt[j * 12 + k]; }
  relative_pose(Pi, Pj, Tg);
#pragma unroll
  for (int k = 0; k < 12; ++k) { Pi[k] = pred[i * 12 + k]; Pj[k] = pred[j * 12 + k]; }
  relative_pose(Pi, Pj, Tp);
  double tr = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) tr = tr + Tg[4 * (k / 3) + k % 3] * Tp[4 * (k / 3) + k % 3];
  const double tg[3] = {Tg[3], Tg[7], Tg[11]}, tp[3] = {Tp[3], Tp[7], Tp[11]};
  const double d2 = (1.0 + tr) * 0.25;
  const double loss_q = fmax(1.0 - d2, kAngleEps);
  out_rot[p] = acos(1.0 - 2.0 * loss_q) * kDegrees;
  const double ng = sqrt((tg[0] * tg[0] + tg[1] * tg[1]) + tg[2] * tg[2]) + kAngleEps;
  const double np = sqrt((tp[0] * tp[0] + tp[1] * tp[1]) + tp[2] * tp[2]) + kAngleEps;
  const double dot = ((tp[0] / np) * (tg[0] / ng) + (tp[1] / np) * (tg[1] / ng)) + (tp[2] / np) * (tg[2] / ng);
  const double loss_t = fmax(1.0 - dot * dot, kAngleEps);
  double err = acos(sqrt(1.0 - loss_t));
  if (!isfinite(err)) err = 1e6;
  const double deg = err * kDegrees;
  out_trans[p] = fmin(deg, fabs(180.0 - deg));
}

// ---------------------------------------------------------------------------------------------------- host helpers
inline int launch_fit(const double* src, const double* tgt, const double* wd, const uint8_t* wm, int B, int N, int estimate_scale,
                      double* out_T, uint8_t* out_valid, char* ws, const Sim3Layout& L, const int32_t* active, const int32_t* changed,
                      hipStream_t st) {
  if (L.G == 1) {
    sim3_fit_single_kernel<<<dim3(B), 256, 0, st>>>(src, tgt, wd, wm, N, estimate_scale, out_T, out_valid, active, changed);
    VGG_LAUNCH_CHECK();
    return VGG_OK;
  }
  double* fit1 = (double*)(ws + L.fit1);
  double* fit2 = (double*)(ws + L.fit2);
  sim3_fit_means_kernel<<<dim3(L.G, B), 256, 0, st>>>(src, tgt, wd, wm, N, L.G, fit1, active, changed);
  VGG_LAUNCH_CHECK();
  sim3_fit_moments_kernel<<<dim3(L.G, B), 256, 0, st>>>(src, tgt, wd, wm, N, L.G, fit1, fit2, active, changed);
  VGG_LAUNCH_CHECK();
  sim3_fit_final_kernel<<<dim3(B), 256, 0, st>>>(L.G, estimate_scale, fit1, fit2, out_T, out_valid, active, changed);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

inline int launch_score(const double* src, const double* tgt, const uint8_t* mask, const double* transforms, const uint8_t* valid,
                        const double* max_error, int B, int N, int H, int32_t* counts, double* sums, char* ws, const Sim3Layout& L,
                        const int32_t* active, const int32_t* changed, hipStream_t st) {
  int32_t* pc = (int32_t*)(ws + L.pc);
  double* ps = (double*)(ws + L.ps);
  sim3_score_kernel<<<dim3(L.P, div_up(H, kTile), B), 256, 0, st>>>(src, tgt, mask, transforms, valid, max_error, N, H, L.P, pc, ps,
                                                                   active, changed);
  VGG_LAUNCH_CHECK();
  const long total = (long)B * H;
  sim3_score_reduce_kernel<<<dim3(div_up(total, 256)), 256, 0, st>>>(valid, H, L.P, total, pc, ps, counts, sums, active, changed);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

inline bool sizes_unsupported(int B, int N, int H) {
  return B > kMaxGridYZ || div_up(H, kTile) > kMaxGridYZ || (double)B * (double)(H < 1 ? 1 : H) * score_parts(N) > 2.0e9 ||
         (double)B * (double)N > 2.0e9;
}

}  // namespace vgg

using namespace vgg;

extern "C" {

size_t vggs_sim3_workspace_bytes(int num_problems, int num_points, int num_hypotheses) {
  if (num_problems <= 0 || num_points < 0 || num_hypotheses < 0) return 0;
  return sim3_layout(num_problems, num_points, num_hypotheses).total;
}

int vggs_sim3_fit(const double* src, const double* tgt, const double* weights, int num_problems, int num_points,
                  int estimate_scale, double* out_transform, uint8_t* out_valid, void* workspace, size_t workspace_bytes,
                  void* stream) {
  if (num_problems < 0 || num_points < 0) return VGG_ERR_INVALID_ARGUMENT;
  if (num_problems == 0 || num_points == 0) return VGG_OK;
  if (!src || !tgt || !out_transform || !out_valid) return VGG_ERR_INVALID_ARGUMENT;
  if (sizes_unsupported(num_problems, num_points, 0)) return VGG_ERR_UNSUPPORTED;
  const Sim3Layout L = sim3_layout(num_problems, num_points, 0);
  if (L.G > 1 && (!workspace || workspace_bytes < L.total)) return VGG_ERR_WORKSPACE;
  return launch_fit(src, tgt, weights, nullptr, num_problems, num_points, estimate_scale, out_transform, out_valid, (char*)workspace,
                    L, nullptr, nullptr, (hipStream_t)stream);
}

int vggs_sim3_score(const double* src, const double* tgt, const uint8_t* mask, const double* transforms, const uint8_t* valid,
                    const double* max_error, int num_problems, int num_points, int num_hypotheses, int32_t* out_counts,
                    double* out_residual_sums, void* workspace, size_t workspace_bytes, void* stream) {
  if (num_problems < 0 || num_points < 0 || num_hypotheses < 0) return VGG_ERR_INVALID_ARGUMENT;
  if (num_problems == 0 || num_points == 0 || num_hypotheses == 0) return VGG_OK;
  if (!src || !tgt || !transforms || !valid || !max_error || !out_counts || !out_residual_sums) return VGG_ERR_INVALID_ARGUMENT;
  if (sizes_unsupported(num_problems, num_points, num_hypotheses)) return VGG_ERR_UNSUPPORTED;
  const Sim3Layout L = sim3_layout(num_problems, num_points, num_hypotheses);
  if (!workspace || workspace_bytes < L.total) return VGG_ERR_WORKSPACE;
  return launch_score(src, tgt, mask, transforms, valid, max_error, num_problems, num_points, num_hypotheses, out_counts,
                      out_residual_sums, (char*)workspace, L, nullptr, nullptr, (hipStream_t)stream);
}

int vggs_sim3_ransac(const double* src, const double* tgt, const uint8_t* mask, const double* max_error, const int32_t* samples,
                     int num_problems, int num_points, int num_hypotheses, int lo_rounds, int min_inliers, int estimate_scale,
                     double* out_transform, int32_t* out_num_inliers, uint8_t* out_inlier_mask, double* out_residual_sum,
                     int32_t* out_best_index, int32_t* out_lo_accepted, uint8_t* out_success, int32_t* out_counts,
                     double* out_residual_sums, void* workspace, size_t workspace_bytes, void* stream) {
  const int B = num_problems, N = num_points, H = num_hypotheses;
  if (B < 0 || N < 0 || H < 0 || lo_rounds < 0 || min_inliers < 3) return VGG_ERR_INVALID_ARGUMENT;
  if (B == 0 || N == 0 || H == 0) return VGG_OK;
  if (!src || !tgt || !max_error || !samples || !out_transform || !out_num_inliers || !out_inlier_mask || !out_residual_sum ||
      !out_best_index || !out_lo_accepted || !out_success || ((out_counts == nullptr) != (out_residual_sums == nullptr)))
    return VGG_ERR_INVALID_ARGUMENT;
  if (sizes_unsupported(B, N, H)) return VGG_ERR_UNSUPPORTED;
  const Sim3Layout L = sim3_layout(B, N, H);
  if (!workspace || workspace_bytes < L.total) return VGG_ERR_WORKSPACE;
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  double* hyp = (double*)(ws + L.hyp);
  uint8_t* hvalid = (uint8_t*)(ws + L.hvalid);
  int32_t* counts = out_counts ? out_counts : (int32_t*)(ws + L.counts);
  double* sums = out_residual_sums ? out_residual_sums : (double*)(ws + L.sums);
  double* cand_T = (double*)(ws + L.cand_T);
  uint8_t* cand_valid = (uint8_t*)(ws + L.cand_valid);
  int32_t* cand_count = (int32_t*)(ws + L.cand_count);
  double* cand_sum = (double*)(ws + L.cand_sum);
  int32_t* active = (int32_t*)(ws + L.active);
  int32_t* changed = (int32_t*)(ws + L.changed);
  int32_t* acc_now = (int32_t*)(ws + L.acc_now);
  const dim3 per_point(div_up(N, 256), B), per_problem(div_up(B, 64));

  sim3_minimal_kernel<<<dim3(div_up(H, 64), B), 64, 0, st>>>(src, tgt, mask, samples, N, H, estimate_scale, hyp, hvalid);
  VGG_LAUNCH_CHECK();
  int rc = launch_score(src, tgt, mask, hyp, hvalid, max_error, B, N, H, counts, sums, ws, L, nullptr, nullptr, st);
  if (rc != VGG_OK) return rc;
  sim3_select_kernel<<<dim3(B), 256, 0, st>>>(H, hyp, counts, sums, out_transform, out_num_inliers, out_residual_sum, out_best_index,
                                             out_lo_accepted, active, changed, acc_now);
  VGG_LAUNCH_CHECK();
  sim3_mask_kernel<<<per_point, 256, 0, st>>>(src, tgt, mask, max_error, N, out_transform, 1, active, acc_now, changed, out_inlier_mask);
  VGG_LAUNCH_CHECK();
  for (int round = 0; round < lo_rounds; ++round) {
    rc = launch_fit(src, tgt, nullptr, out_inlier_mask, B, N, estimate_scale, cand_T, cand_valid, ws, L, active, changed, st);
    if (rc != VGG_OK) return rc;
    rc = launch_score(src, tgt, mask, cand_T, cand_valid, max_error, B, N, 1, cand_count, cand_sum, ws, L, active, changed, st);
    if (rc != VGG_OK) return rc;
    sim3_lo_decide_kernel<<<per_problem, 64, 0, st>>>(B, cand_T, cand_valid, cand_count, cand_sum, out_transform, out_num_inliers,
                                                     out_residual_sum, out_lo_accepted, active, changed, acc_now);
    VGG_LAUNCH_CHECK();
    sim3_mask_kernel<<<per_point, 256, 0, st>>>(src, tgt, mask, max_error, N, out_transform, 0, active, acc_now, changed,
                                               out_inlier_mask);
    VGG_LAUNCH_CHECK();
  }
  sim3_final_kernel<<<per_problem, 64, 0, st>>>(B, min_inliers, out_transform, out_num_inliers, out_residual_sum, out_best_index,
                                               out_success, active);
  VGG_LAUNCH_CHECK();
  sim3_clear_failed_kernel<<<per_point, 256, 0, st>>>(N, active, out_inlier_mask);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vggs_pose_pair_errors(const double* pred, const double* gt, int num_cameras, double* out_rot_deg, double* out_trans_deg,
                          void* stream) {
  if (num_cameras < 0) return VGG_ERR_INVALID_ARGUMENT;
  if (num_cameras < 2) return VGG_OK;
  if (!pred || !gt || !out_rot_deg || !out_trans_deg) return VGG_ERR_INVALID_ARGUMENT;
  const long pairs = (long)num_cameras * (num_cameras - 1) / 2;
  if (pairs > 2147483647L) return VGG_ERR_UNSUPPORTED;
  pose_pair_errors_kernel<<<dim3(div_up(pairs, 256)), 256, 0, (hipStream_t)stream>>>(pred, gt, num_cameras, pairs, out_rot_deg,
                                                                                    out_trans_deg);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

}  // extern "C"
