// Dense depth alignment, the `dense_depth` stage of the reference's demo:
//   extract_sparse_depth_and_point_from_reconstruction   vggsfm/runners/runner.py:744-772
//   align_dense_depth_maps                                vggsfm/utils/utils.py:635-770
// Three kernels: the per-observation projection of the sparse model, the per-image RANSAC fit of
// disparity ~ scale * d + shift (scikit-learn 1.7 RANSACRegressor + LinearRegression semantics, one workgroup per
// image), and the per-pixel rescale / inversion (+ back-projection of the valid pixels to the world).
// Compiled with -ffp-contract=off: the depth maps are compared bit-for-bit with the reference's numpy float32 arithmetic,
// and the 2-point hypotheses restate LAPACK's float32 least squares operation by operation.
#include <algorithm>

#include "common.hpp"
#include "scan.hpp"
#include "../../include/vggsfm_amd.h"

namespace vgg {
namespace {

constexpr int kAlignThreads = 512;
constexpr int kAlignWaves = kAlignThreads / kWave;
constexpr int kRadixBins = 256;

// status codes of vgg_depth_align (vggsfm_amd/dense_depth.py maps them to the reference's errors)
enum : int { kAlignOk = 0, kAlignNoPoints = 1, kAlignIllPosed = 2, kAlignNoConsensus = 3, kAlignTooFewKept = 4,
             kAlignDrawsExhausted = 5, kAlignBadDraw = 6 };

// ------------------------------------------------------------------ sparse depth
// out row o: image obs_image[o] sees point row obs_point[o] (id point_id[o]); rows are already grouped by image.
// pose (S,3,4) [R|t], cam (S,4) f, cx, cy, k (k = 0 for SIMPLE_PINHOLE).  Same operation order as
// pycolmap_compat: p = R X + t, uv = f * (p01 / p2) * (1 + k r2) + c.
__global__ __launch_bounds__(256) void sparse_depth_kernel(const double* __restrict__ xyz, const int32_t* __restrict__ obs_point,
                                                           const int32_t* __restrict__ obs_image,
                                                           const int64_t* __restrict__ point_id, const double* __restrict__ pose,
                                                           const double* __restrict__ cam, long O, double* __restrict__ uvd,
                                                           double* __restrict__ xyzid) {
  for (long o = blockIdx.x * (long)blockDim.x + threadIdx.x; o < O; o += (long)gridDim.x * blockDim.x) {
    const int p = obs_point[o], s = obs_image[o];
    const double* P = pose + 12 * (size_t)s;
    const double* c = cam + 4 * (size_t)s;
    const double X = xyz[3 * (size_t)p], Y = xyz[3 * (size_t)p + 1], Z = xyz[3 * (size_t)p + 2];
    const double p0 = (P[0] * X + P[1] * Y + P[2] * Z) + P[3];
    const double p1 = (P[4] * X + P[5] * Y + P[6] * Z) + P[7];
    const double p2 = (P[8] * X + P[9] * Y + P[10] * Z) + P[11];
    const double u = p0 / p2, v = p1 / p2;
    const double d = 1.0 + c[3] * (u * u + v * v);
    uvd[3 * o] = c[0] * u * d + c[1];
    uvd[3 * o + 1] = c[0] * v * d + c[2];
    uvd[3 * o + 2] = p2;
    xyzid[4 * o] = X;
    xyzid[4 * o + 1] = Y;
    xyzid[4 * o + 2] = Z;
    xyzid[4 * o + 3] = (double)point_id[o];
  }
}

// ------------------------------------------------------------------ block helpers (kAlignThreads threads)
__device__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();
  if (lane_id() == 0) red[threadIdx.x / kWave] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < kAlignWaves; ++w) t += red[w];
  return t;
}

__device__ long block_sum_l(long v, long* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();
  if (lane_id() == 0) red[threadIdx.x / kWave] = v;
  __syncthreads();
  long t = 0;
  for (int w = 0; w < kAlignWaves; ++w) t += red[w];
  return t;
}

// k-th smallest (0-based) of M positive doubles: radix select on the IEEE bit pattern (monotone for x >= 0)
__device__ double block_select(const double* __restrict__ y, int M, int k, unsigned* hist, int* sel) {
  unsigned long long prefix = 0, mask = 0;
  for (int shift = 56; shift >= 0; shift -= 8) {
    __syncthreads();
    for (int b = threadIdx.x; b < kRadixBins; b += kAlignThreads) hist[b] = 0;
    __syncthreads();
    for (int j = threadIdx.x; j < M; j += kAlignThreads) {
      const unsigned long long bits = (unsigned long long)__double_as_longlong(y[j]);
      if ((bits & mask) == prefix) atomicAdd(&hist[(bits >> shift) & 255ull], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int cum = 0, b = 0;
      for (; b < kRadixBins - 1; ++b) {
        if (cum + (int)hist[b] > k) break;
        cum += (int)hist[b];
      }
      sel[0] = b;
      sel[1] = k - cum;
    }
    __syncthreads();
    prefix |= (unsigned long long)sel[0] << shift;
    mask |= 255ull << shift;
    k = sel[1];
  }
  return __longlong_as_double((long long)prefix);
}

// LinearRegression().fit on two points as scikit-learn 1.7 computes it: X and y in float32, centred on their float32
// means, then LAPACK sgelsd on the 2x1 column -- a Householder reflection (slarfg), Q^T b (slarf) and the 1x1 solve
// b / R11 (slascl multiplies by 1 / R11).  coef = 0 when the centred column is zero (the two x are equal).
__device__ __forceinline__ void fit_two_points(float x0, float x1, float y0, float y1, float& coef, float& icpt) {
  const float xo = (x0 + x1) / 2.0f, yo = (y0 + y1) / 2.0f;
  const float a1 = x0 - xo, a2 = x1 - xo, b1 = y0 - yo, b2 = y1 - yo;
  float c;
  if (a2 == 0.0f) {
    c = (a1 == 0.0f) ? 0.0f : b1 * (1.0f / a1);        // slarfg: xnorm == 0 -> tau = 0, R11 = a1
  } else {
    const float w = fmaxf(fabsf(a1), fabsf(a2)), z = fminf(fabsf(a1), fabsf(a2));
    const float q = z / w;
    const float nrm = w * sqrtf(1.0f + q * q);           // slapy2
    const float beta = -copysignf(nrm, a1);
    const float tau = (beta - a1) / beta;
    const float v2 = a2 * (1.0f / (a1 - beta));
    const float wd = b1 + v2 * b2;
    const float qb1 = b1 - tau * wd;
    c = qb1 * (1.0f / beta);
  }
  coef = c;
  icpt = yo - xo * c;
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// sklearn.linear_model._ransac._dynamic_max_trials with min_samples = 2, stop_probability = 0.99
__device__ double dynamic_max_trials(int n_inliers, int n_samples) {
  const double eps = 2.220446049250313e-16;
  const double ratio = (double)n_inliers / (double)n_samples;
  const double nom = fmax(eps, 1.0 - 0.99);
  const double denom = fmax(eps, 1.0 - ratio * ratio);
  if (denom == 1.0) return __builtin_inf();
  return fabs(ceil(log(nom) / log(denom)));
}

struct AlignShared {
  double red[kAlignWaves];
  long redl[kAlignWaves];
  int wave_cnt[kAlignWaves];
  unsigned hist[kRadixBins];
  int sel[2];
  int cnt[kAlignWaves];
  double score[kAlignWaves];
  float hc[kAlignWaves], hb[kAlignWaves];
  int bad[kAlignWaves];
  // replay state (lane 0 of wave 0 writes, everyone reads after a barrier)
  int n_best, n_trials, stop, status;
  double score_best, max_trials;
  float best_c, best_b;
};

// One workgroup per image.  wx / wy / widx: per-observation workspace (the kept (x, y) pairs of image i are compacted to
// rows obs_ptr[i] .. obs_ptr[i] + M_i, in observation order, widx = their observation row).
__global__ __launch_bounds__(kAlignThreads) void depth_align_kernel(
    const float* __restrict__ disp, const int64_t* __restrict__ disp_off, const int32_t* __restrict__ Hs,
    const int32_t* __restrict__ Ws, const double* __restrict__ uvd, const int64_t* __restrict__ obs_ptr,
    const int32_t* __restrict__ draws, int num_draws, unsigned long long seed, int max_trials, float* __restrict__ wx,
    double* __restrict__ wy, int32_t* __restrict__ widx, float* __restrict__ scale, float* __restrict__ shift,
    int32_t* __restrict__ n_trials_out, int32_t* __restrict__ n_inliers_out, int32_t* __restrict__ n_kept_out,
    int32_t* __restrict__ status_out, uint8_t* __restrict__ kept, uint8_t* __restrict__ inlier) {
  __shared__ AlignShared sh;
  const int img = blockIdx.x, tid = threadIdx.x, wave = tid / kWave, lane = lane_id();
  const long a = obs_ptr[img], b = obs_ptr[img + 1];
  const float* dm = disp + disp_off[img];
  const int H = Hs[img], W = Ws[img];
  float* X = wx + a;
  double* Y = wy + a;
  int32_t* I = widx + a;
  if (tid == 0) { scale[img] = 0.0f; shift[img] = 0.0f; n_trials_out[img] = 0; n_inliers_out[img] = 0; n_kept_out[img] = 0; }
  if (b <= a) {
    if (tid == 0) status_out[img] = kAlignNoPoints;
    return;
  }
  // ---- gather + filter (utils.py:665-688): in-bounds by round-half-even, sampled disparity > 0, depth clipped
  int M = 0;
  long nonfinite = 0;
  for (long base = a; base < b; base += kAlignThreads) {
    const long o = base + tid;
    bool keep = false;
    float x = 0.0f;
    double y = 0.0;
    if (o < b) {
      const double ru = rint(uvd[3 * o]), rv = rint(uvd[3 * o + 1]);
      if (ru >= 0.0 && ru < (double)W && rv >= 0.0 && rv < (double)H) {
        x = dm[(long)rv * W + (long)ru];
        if (x > 0.0f) {
          keep = true;
          const double z = uvd[3 * o + 2];
          y = 1.0 / fmin(fmax(z, 0.0001), 10000.0);     // np.clip(depth, 1e-4, 1e4); a NaN depth: ill-posed
          if (!(z == z) || !isfinite(x)) ++nonfinite;
        }
      }
      kept[o] = keep ? 1 : 0;
      inlier[o] = 0;
    }
    int total;
    const int pos = block_scan_flag<kAlignWaves>(keep, sh.wave_cnt, &total);
    if (keep) {
      X[M + pos] = x;
      Y[M + pos] = y;
      I[M + pos] = (int32_t)(o - a);
    }
    M += total;
  }
  nonfinite = block_sum_l(nonfinite, sh.redl);
  if (tid == 0) n_kept_out[img] = M;
  if (M < 2) {
    if (tid == 0) status_out[img] = kAlignTooFewKept;
    return;
  }
  if (nonfinite) {
    if (tid == 0) status_out[img] = kAlignIllPosed;
    return;
  }
  __syncthreads();   // compacted rows visible to the whole block
  // ---- numpy median (mean of the two middle values for even M), threshold = median / 30
  double med = block_select(Y, M, (M - 1) / 2, sh.hist, sh.sel);
  if ((M & 1) == 0) med = (med + block_select(Y, M, M / 2, sh.hist, sh.sel)) / 2.0;
  const double thr = med / 30.0;
  if (!(thr > 0.0)) {
    if (tid == 0) status_out[img] = kAlignIllPosed;
    return;
  }
  // ---- RANSAC (sklearn/linear_model/_ransac.py, fit): every wave scores one hypothesis of the current round; lane 0 of
  // wave 0 then replays the round's (count, score) pairs in draw order, exactly as the sequential loop would
  if (tid == 0) {
    sh.n_best = 1; sh.n_trials = 0; sh.stop = 0; sh.status = kAlignOk;
    sh.score_best = -__builtin_inf(); sh.max_trials = (double)max_trials;
    sh.best_c = 0.0f; sh.best_b = 0.0f;
  }
  __syncthreads();
  for (int round = 0;; ++round) {
    if (sh.stop) break;
    const int t = round * kAlignWaves + wave;
    int cnt = -1;
    double score = 0.0;
    float hc = 0.0f, hb = 0.0f;
    int bad = 0;
    if ((double)t < sh.max_trials && (draws == nullptr || t < num_draws)) {
      int i, j;
      if (draws) {
        const int32_t* dr = draws + 2 * ((size_t)img * num_draws + t);
        i = dr[0];
        j = dr[1];
      } else {
        const unsigned long long h1 = mix64(seed ^ mix64(((unsigned long long)img << 32) | (unsigned)t));
        const unsigned long long h2 = mix64(h1);
        i = (int)(h1 % (unsigned long long)M);
        j = (int)(h2 % (unsigned long long)(M - 1));
        j += (j >= i);
      }
      if (i < 0 || i >= M || j < 0 || j >= M) {
        bad = 1;
      } else {
        fit_two_points(X[i], X[j], (float)Y[i], (float)Y[j], hc, hb);
        int c = 0;
        double sy = 0.0, ssr = 0.0;
        for (int k = lane; k < M; k += kWave) {
          const float pred = X[k] * hc + hb;
          const double r = Y[k] - (double)pred;
          const double r2 = r * r;
          if (r2 <= thr) { ++c; sy += Y[k]; ssr += r2; }
        }
        c = wave_sum_i(c);
        sy = wave_sum(sy);
        ssr = wave_sum(ssr);
        cnt = c;
        if (c < 2) {
          score = __builtin_nan("");      // r2_score of fewer than two samples
        } else {
          const double mean = sy / (double)c;
          double sst = 0.0;
          for (int k = lane; k < M; k += kWave) {
            const float pred = X[k] * hc + hb;
            const double r = Y[k] - (double)pred;
            if (r * r <= thr) { const double e = Y[k] - mean; sst += e * e; }
          }
          sst = wave_sum(sst);
          score = (sst == 0.0) ? (ssr == 0.0 ? 1.0 : 0.0) : 1.0 - ssr / sst;
        }
      }
    }
    if (lane == 0) { sh.cnt[wave] = cnt; sh.score[wave] = score; sh.hc[wave] = hc; sh.hb[wave] = hb; sh.bad[wave] = bad; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 0; w < kAlignWaves; ++w) {
        const int tt = round * kAlignWaves + w;
        if (!((double)sh.n_trials < sh.max_trials)) { sh.stop = 1; break; }
        if (draws && tt >= num_draws) { sh.status = kAlignDrawsExhausted; sh.stop = 1; break; }
        if (sh.bad[w]) { sh.status = kAlignBadDraw; sh.stop = 1; break; }
        sh.n_trials += 1;
        const int c = sh.cnt[w];
        if (c < sh.n_best) continue;
        if (c == sh.n_best && sh.score[w] < sh.score_best) continue;
        sh.n_best = c;
        sh.score_best = sh.score[w];
        sh.best_c = sh.hc[w];
        sh.best_b = sh.hb[w];
        sh.status = -1;                                  // (marks "a consensus set exists"; reset below)
        sh.max_trials = fmin(sh.max_trials, dynamic_max_trials(c, M));
      }
      if (!((double)sh.n_trials < sh.max_trials)) sh.stop = 1;
    }
    __syncthreads();
  }
  const int status = sh.status;
  if (tid == 0) n_trials_out[img] = sh.n_trials;
  if (status != -1) {                                    // no hypothesis accepted, or the draws ran out / were invalid
    if (tid == 0) status_out[img] = (status == kAlignOk) ? kAlignNoConsensus : status;
    return;
  }
  // ---- inliers of the best hypothesis, then LinearRegression on them (two-pass, float64 on the float32 data)
  const float bc = sh.best_c, bb = sh.best_b;
  long n_in = 0;
  double sx = 0.0, sy = 0.0;
  for (int k = tid; k < M; k += kAlignThreads) {
    const float pred = X[k] * bc + bb;
    const double r = Y[k] - (double)pred;
    if (r * r <= thr) {
      inlier[a + I[k]] = 1;
      ++n_in;
      sx += (double)X[k];
      sy += (double)(float)Y[k];
    }
  }
  n_in = block_sum_l(n_in, sh.redl);
  sx = block_sum(sx, sh.red);
  sy = block_sum(sy, sh.red);
  const double xm = sx / (double)n_in, ym = sy / (double)n_in;
  double sxy = 0.0, sxx = 0.0;
  for (int k = tid; k < M; k += kAlignThreads) {
    const float pred = X[k] * bc + bb;
    const double r = Y[k] - (double)pred;
    if (r * r <= thr) {
      const double dx = (double)X[k] - xm, dy = (double)(float)Y[k] - ym;
      sxy += dx * dy;
      sxx += dx * dx;
    }
  }
  sxy = block_sum(sxy, sh.red);
  sxx = block_sum(sxx, sh.red);
  if (tid == 0) {
    const double coef = (sxx > 0.0) ? sxy / sxx : 0.0;
    scale[img] = (float)coef;
    shift[img] = (float)(ym - xm * coef);
    n_inliers_out[img] = (int32_t)n_in;
    status_out[img] = kAlignOk;
  }
}

// ------------------------------------------------------------------ apply (utils.py:720-735), numpy float32 semantics:
// nonzero d -> d * scale + shift (float32 ops, scale / shift float32 scalars), outside (0, 1e4] -> 0, depth = 1 / d (inf -> 0)
__global__ __launch_bounds__(256) void depth_apply_kernel(float* __restrict__ disp, float* __restrict__ depth,
                                                          const int64_t* __restrict__ off, const int32_t* __restrict__ Hs,
                                                          const int32_t* __restrict__ Ws, const float* __restrict__ scale,
                                                          const float* __restrict__ shift) {
  const int img = blockIdx.y;
  const long n = (long)Hs[img] * Ws[img];
  const float s = scale[img], t = shift[img];
  float* dm = disp + off[img];
  float* dp = depth + off[img];
  for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < n; p += (long)gridDim.x * blockDim.x) {
    float d = dm[p];
    if (d != 0.0f) d = d * s + t;
    if (!(d > 0.0f && d <= 10000.0f)) d = 0.0f;
    dm[p] = d;
    float z = 0.0f;
    if (d != 0.0f) {
      z = 1.0f / d;
      if (isinf(z)) z = 0.0f;
    }
    dp[p] = z;
  }
}

// ------------------------------------------------------------------ back-projection of the valid pixels (utils.py:727-762)
// pixel p of image pix_image[n] -> x = p % W, y = p / W (integer grid); cam_from_img as pycolmap_compat.Camera restates
// COLMAP (per point here: Newton with a central-difference Jacobian, <= 100 iterations, stop at |step|^2 < 1e-10), times
// the depth, then world = R^T (.) - R^T t given as inv_pose (S,3,4).
__device__ __forceinline__ void radial(double k, double u, double v, double& ou, double& ov) {
  const double f = 1.0 + k * (u * u + v * v);
  ou = u * f;
  ov = v * f;
}

__global__ __launch_bounds__(256) void unproject_kernel(const int64_t* __restrict__ pix, const int32_t* __restrict__ pix_image,
                                                        long N, const float* __restrict__ depth, const int64_t* __restrict__ off,
                                                        const int32_t* __restrict__ Ws, const double* __restrict__ cam,
                                                        const double* __restrict__ inv_pose, double* __restrict__ xyz) {
  for (long n = blockIdx.x * (long)blockDim.x + threadIdx.x; n < N; n += (long)gridDim.x * blockDim.x) {
    const int s = pix_image[n];
    const long p = pix[n];
    const int W = Ws[s];
    const double px = (double)(p % W), py = (double)(p / W);
    const double* c = cam + 4 * (size_t)s;
    const double x0 = (px - c[1]) / c[0], y0 = (py - c[2]) / c[0];
    double u = x0, v = y0;
    const double k = c[3];
    if (k != 0.0) {
      for (int it = 0; it < 100; ++it) {
        const double su = fmax(2.220446049250313e-16, fabs(1e-6 * u)), sv = fmax(2.220446049250313e-16, fabs(1e-6 * v));
        double a0, a1, b0, b1;
        radial(k, u + su, v, a0, a1);
        radial(k, u - su, v, b0, b1);
        const double J00 = (a0 - b0) / (2 * su), J10 = (a1 - b1) / (2 * su);
        radial(k, u, v + sv, a0, a1);
        radial(k, u, v - sv, b0, b1);
        const double J01 = (a0 - b0) / (2 * sv), J11 = (a1 - b1) / (2 * sv);
        double du, dv;
        radial(k, u, v, du, dv);
        double r0 = du - x0, r1 = dv - y0;
        // 2x2 LU with partial pivoting (LAPACK gesv)
        double m00 = J00, m01 = J01, m10 = J10, m11 = J11;
        if (fabs(m10) > fabs(m00)) {
          double tmp = m00; m00 = m10; m10 = tmp;
          tmp = m01; m01 = m11; m11 = tmp;
          tmp = r0; r0 = r1; r1 = tmp;
        }
        const double l = m10 / m00;
        const double s1 = (r1 - l * r0) / (m11 - l * m01);
        const double s0 = (r0 - m01 * s1) / m00;
        u -= s0;
        v -= s1;
        if (s0 * s0 + s1 * s1 < 1e-10) break;
      }
    }
    const double z = (double)depth[off[s] + p];
    const double cx = u * z, cy = v * z, cz = 1.0 * z;
    const double* T = inv_pose + 12 * (size_t)s;
    xyz[3 * n] = (T[0] * cx + T[1] * cy + T[2] * cz) + T[3];
    xyz[3 * n + 1] = (T[4] * cx + T[5] * cy + T[6] * cz) + T[7];
    xyz[3 * n + 2] = (T[8] * cx + T[9] * cy + T[10] * cz) + T[11];
  }
}

}  // namespace
}  // namespace vgg

using namespace vgg;

extern "C" {

int vgg_sparse_depth(const double* xyz, const int32_t* obs_point, const int32_t* obs_image, const int64_t* point_id,
                     const double* pose, const double* cam, long num_obs, double* uvd, double* xyzid, void* stream) {
  if (num_obs < 0) return VGG_ERR_INVALID_ARGUMENT;
  if (num_obs == 0) return VGG_OK;
  if (!xyz || !obs_point || !obs_image || !point_id || !pose || !cam || !uvd || !xyzid) return VGG_ERR_INVALID_ARGUMENT;
  const int grid = (int)std::min<long>((num_obs + 255) / 256, 4096);
  sparse_depth_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(xyz, obs_point, obs_image, point_id, pose, cam, num_obs, uvd,
                                                               xyzid);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

size_t vgg_depth_align_workspace_bytes(long num_obs) {
  return (size_t)num_obs * (sizeof(double) + sizeof(float) + sizeof(int32_t)) + 64;
}

int vgg_depth_align(const float* disp, const int64_t* disp_off, const int32_t* heights, const int32_t* widths,
                    const double* uvd, const int64_t* obs_ptr, int num_images, long num_obs, const int32_t* draws,
                    int num_draws, unsigned long long seed, int max_trials, float* scale, float* shift, int32_t* n_trials,
                    int32_t* n_inliers, int32_t* n_kept, int32_t* status, uint8_t* kept, uint8_t* inlier, void* workspace,
                    size_t workspace_bytes, void* stream) {
  if (num_images < 0 || num_obs < 0 || max_trials < 0 || (draws && num_draws < 0)) return VGG_ERR_INVALID_ARGUMENT;
  if (num_images == 0) return VGG_OK;
  if (!disp || !disp_off || !heights || !widths || !obs_ptr || !scale || !shift || !n_trials || !n_inliers || !n_kept ||
      !status || (num_obs > 0 && (!uvd || !kept || !inlier)))
    return VGG_ERR_INVALID_ARGUMENT;
  if (num_obs > 0x7fffffffL) return VGG_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < vgg_depth_align_workspace_bytes(num_obs)) return VGG_ERR_WORKSPACE;
  double* wy = (double*)workspace;
  float* wx = (float*)(wy + num_obs);
  int32_t* widx = (int32_t*)(wx + num_obs);
  depth_align_kernel<<<num_images, kAlignThreads, 0, (hipStream_t)stream>>>(
      disp, disp_off, heights, widths, uvd, obs_ptr, draws, num_draws, seed, max_trials, wx, wy, widx, scale, shift,
      n_trials, n_inliers, n_kept, status, kept, inlier);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vgg_depth_apply(float* disp, float* depth, const int64_t* disp_off, const int32_t* heights, const int32_t* widths,
                    int num_images, long max_pixels, const float* scale, const float* shift, void* stream) {
  if (num_images < 0 || max_pixels < 0) return VGG_ERR_INVALID_ARGUMENT;
  if (num_images == 0 || max_pixels == 0) return VGG_OK;
  if (!disp || !depth || !disp_off || !heights || !widths || !scale || !shift) return VGG_ERR_INVALID_ARGUMENT;
  if (num_images > 65535) return VGG_ERR_UNSUPPORTED;
  // ~2048 workgroups in total, grid-stride over the pixels of an image (max_pixels: the largest H * W of the batch)
  const dim3 grid((unsigned)std::max<long>(1, std::min<long>((max_pixels + 255) / 256, std::max(1, 2048 / num_images))),
                  num_images);
  depth_apply_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(disp, depth, disp_off, heights, widths, scale, shift);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vgg_depth_unproject(const int64_t* pixels, const int32_t* pixel_image, long num_pixels, const float* depth,
                        const int64_t* disp_off, const int32_t* widths, const double* cam, const double* inv_pose,
                        double* xyz, void* stream) {
  if (num_pixels < 0) return VGG_ERR_INVALID_ARGUMENT;
  if (num_pixels == 0) return VGG_OK;
  if (!pixels || !pixel_image || !depth || !disp_off || !widths || !cam || !inv_pose || !xyz) return VGG_ERR_INVALID_ARGUMENT;
  const int grid = (int)std::min<long>((num_pixels + 255) / 256, 8192);
  unproject_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(pixels, pixel_image, num_pixels, depth, disp_off, widths, cam,
                                                            inv_pose, xyz);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

}  // extern "C"
