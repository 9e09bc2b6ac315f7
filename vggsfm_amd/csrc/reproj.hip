// Reprojection video, the `make_reproj_video` stage of the reference's demo:
//   create_video_with_reprojections   vggsfm/utils/utils.py:428-546
//   filter_invisible_reprojections    vggsfm/utils/utils.py:393-425
// Three entries: the colour statistics over all points (NumPy median / percentile by radix select on order-preserving
// 64-bit keys), the per-observation centre, colour and per-pixel visibility winner (integer atomics on a per-frame grid,
// order-independent, so bit-reproducible), and the per-pixel compositing of the winning circles onto the padded BGR
// canvas (an integer 4x4 sub-sample raster rule in place of OpenCV's anti-aliased fill).
// Compiled with -ffp-contract=off: the statistics and colour indices restate numpy's float64 arithmetic bit for bit.
#include <algorithm>

#include "common.hpp"
#include "../../include/vggsfm_amd.h"

namespace vgg {
namespace {

constexpr int kStatsThreads = 1024;
constexpr int kRadixBins = 256;
constexpr unsigned long long kSign = 0x8000000000000000ull;
constexpr uint32_t kEmpty = 0xffffffffu;
constexpr int kTileW = 32, kTileH = 8;        // draw: one 256-thread workgroup per 32 x 8 canvas pixels

enum : int { kDisToCenter = 0, kDisToOrigin = 1, kPointOrder = 2 };
// workspace accumulators of vgg_reproj_stats
enum : int { kAccMin = 0, kAccMax = 1, kAccNan = 2, kAccMaxId = 3, kAccColNan = 4, kAccWords = 8 };

// total order of the doubles (NaN aside): -inf < ... < -0 < +0 < ... < +inf
__device__ __forceinline__ unsigned long long order_key(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b & kSign) ? ~b : (b | kSign);
}
__device__ __forceinline__ double order_key_inv(unsigned long long k) {
  return __longlong_as_double((long long)((k & kSign) ? (k & ~kSign) : ~k));
}
// visibility key: np.argmin semantics -- -0.0 == +0.0, and a NaN wins (argmin returns the first NaN)
__device__ __forceinline__ unsigned long long depth_key(double d) {
  if (d != d) return 0ull;
  return order_key(d == 0.0 ? 0.0 : d);
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, (unsigned long long)__shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, (unsigned long long)__shfl_xor(v, off, 64));
  return v;
}

// k-th smallest (0-based) of n keys, one workgroup of kStatsThreads: 8 passes of an 8-bit digit histogram
__device__ unsigned long long block_select_key(const unsigned long long* __restrict__ keys, long n, long k, unsigned* hist,
                                               long* sel) {
  unsigned long long prefix = 0, mask = 0;
  for (int shift = 56; shift >= 0; shift -= 8) {
    __syncthreads();
    for (int b = threadIdx.x; b < kRadixBins; b += blockDim.x) hist[b] = 0;
    __syncthreads();
    for (long j = threadIdx.x; j < n; j += blockDim.x) {
      const unsigned long long key = keys[j];
      if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255ull], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      long cum = 0;
      int b = 0;
      for (; b < kRadixBins - 1; ++b) {
        if (cum + (long)hist[b] > k) break;
        cum += (long)hist[b];
      }
      sel[0] = b;
      sel[1] = k - cum;
    }
    __syncthreads();
    prefix |= (unsigned long long)sel[0] << shift;
    mask |= 255ull << shift;
    k = sel[1];
  }
  return prefix;
}

// ------------------------------------------------------------------ colour statistics (utils.py:470-485)
// keys (3, P): column keys for the medians; acc initialised here (the later launches of the same call read it)
__global__ __launch_bounds__(256) void stats_keys_kernel(const double* __restrict__ xyz, long P,
                                                         unsigned long long* __restrict__ keys,
                                                         unsigned long long* __restrict__ acc) {
  if (blockIdx.x == 0 && threadIdx.x < kAccWords)
    acc[threadIdx.x] = threadIdx.x == kAccMin ? ~0ull : (threadIdx.x == kAccMaxId ? (unsigned long long)INT64_MIN : 0ull);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < P; i += (long)gridDim.x * blockDim.x) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double x = xyz[3 * i + c];
      keys[c * P + i] = order_key(x);
      if (x != x) atomicOr(&acc[kAccColNan + c], 1ull);
    }
  }
}

// np.median(points3D, axis=0): one workgroup per axis; the middle element, or (a + b) / 2 of the two middle ones
__global__ __launch_bounds__(kStatsThreads) void stats_median_kernel(const unsigned long long* __restrict__ keys, long P,
                                                                     const unsigned long long* __restrict__ acc,
                                                                     double* __restrict__ stats) {
  __shared__ unsigned hist[kRadixBins];
  __shared__ long sel[2];
  const int c = blockIdx.x;
  const unsigned long long* k = keys + c * P;
  double med;
  if (acc[kAccColNan + c]) {
    med = __builtin_nan("");
  } else {
    med = order_key_inv(block_select_key(k, P, (P - 1) / 2, hist, sel));
    if ((P & 1) == 0) med = (med + order_key_inv(block_select_key(k, P, P / 2, hist, sel))) / 2.0;
  }
  if (threadIdx.x == 0) stats[c] = med;
}

// distances to the centre (stats[0..2]; zero for dis_to_origin: x - 0.0 is x, and the norm is the same), as
// np.linalg.norm: sqrt((dx*dx + dy*dy) + dz*dz); their keys for the percentile, min / max / NaN; or the largest point id
__global__ __launch_bounds__(256) void stats_dist_kernel(const double* __restrict__ xyz, const int64_t* __restrict__ point_id,
                                                         long P, int mode, const double* __restrict__ stats,
                                                         unsigned long long* __restrict__ keys,
                                                         unsigned long long* __restrict__ acc) {
  unsigned long long lo = ~0ull, hi = 0ull, nan = 0ull;
  long long maxid = INT64_MIN;
  const double m0 = stats[0], m1 = stats[1], m2 = stats[2];
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < P; i += (long)gridDim.x * blockDim.x) {
    if (mode == kPointOrder) {
      maxid = max(maxid, (long long)point_id[i]);
      continue;
    }
    const double dx = xyz[3 * i] - m0, dy = xyz[3 * i + 1] - m1, dz = xyz[3 * i + 2] - m2;
    const double d = sqrt((dx * dx + dy * dy) + dz * dz);
    const unsigned long long key = order_key(d);
    keys[i] = key;
    if (d != d) {
      nan = 1ull;
    } else {
      lo = min(lo, key);
      hi = max(hi, key);
    }
  }
  lo = wave_min_u64(lo);
  hi = wave_max_u64(hi);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    maxid = max(maxid, (long long)__shfl_xor(maxid, off, 64));
    nan |= (unsigned long long)__shfl_xor(nan, off, 64);
  }
  if (lane_id() == 0) {
    if (mode == kPointOrder) {
      atomicMax((long long*)&acc[kAccMaxId], maxid);
    } else {
      atomicMin(&acc[kAccMin], lo);
      atomicMax(&acc[kAccMax], hi);
      if (nan) atomicOr(&acc[kAccNan], 1ull);
    }
  }
}

// min_dis / max_dis: np.percentile(distances, 95) (numpy 2.2, method "linear": virtual index (n - 1) * 0.95, _lerp with
// its t >= 0.5 branch) for dis_to_center, the max for dis_to_origin; a NaN distance makes both NaN, as numpy's do
__global__ __launch_bounds__(kStatsThreads) void stats_final_kernel(const unsigned long long* __restrict__ keys, long P,
                                                                    int mode, const unsigned long long* __restrict__ acc,
                                                                    double* __restrict__ stats) {
  __shared__ unsigned hist[kRadixBins];
  __shared__ long sel[2];
  if (mode == kPointOrder) {
    if (threadIdx.x == 0) {
      stats[0] = stats[1] = stats[2] = 0.0;
      stats[3] = stats[4] = 0.0;
      stats[5] = (double)(long long)acc[kAccMaxId];
    }
    return;
  }
  const double nanv = __builtin_nan("");
  const bool has_nan = acc[kAccNan] != 0;
  double lo = has_nan ? nanv : order_key_inv(acc[kAccMin]);
  double hi;
  if (has_nan) {
    hi = nanv;
  } else if (mode == kDisToOrigin) {
    hi = order_key_inv(acc[kAccMax]);
  } else {
    const double vi = (double)(P - 1) * 0.95;
    long prev, next;
    if (vi >= (double)(P - 1)) {
      prev = next = P - 1;
    } else {
      prev = (long)floor(vi);
      next = prev + 1;
    }
    const double prev_f = (vi >= (double)(P - 1)) ? -1.0 : (double)prev;   // numpy keeps -1 for "above bounds"
    const double t = vi - prev_f;
    const double a = order_key_inv(block_select_key(keys, P, prev, hist, sel));
    const double b = (next == prev) ? a : order_key_inv(block_select_key(keys, P, next, hist, sel));
    const double diff = b - a;
    hi = (t >= 0.5) ? b - diff * (1.0 - t) : a + diff * t;
  }
  if (threadIdx.x == 0) {
    if (mode == kDisToOrigin) stats[0] = stats[1] = stats[2] = 0.0;
    stats[3] = lo;
    stats[4] = hi;
    stats[5] = 0.0;
  }
}

// ------------------------------------------------------------------ visibility (utils.py:393-425, 499-526)
// frame f of the chunk owns observations obs_range[f][0] .. obs_range[f][1]; its grid window is (H + 2r) x (W + 2r) cells
// starting at grid_off[f] - grid_off[frame_begin], cell (gx, gy) = centre (gx - r, gy - r)
struct FrameObs {
  long a, b, base;
  int gw, gh;
};
__device__ __forceinline__ FrameObs frame_obs(const int64_t* obs_range, const int32_t* Hs, const int32_t* Ws,
                                              const int64_t* grid_off, int frame_begin, int r) {
  const int f = frame_begin + blockIdx.y;
  FrameObs o;
  o.a = obs_range[2 * f];
  o.b = obs_range[2 * f + 1];
  o.base = grid_off[f] - grid_off[frame_begin];
  o.gw = Ws[f] + 2 * r;
  o.gh = Hs[f] + 2 * r;
  return o;
}

// colour index of one observation (utils.py:503-516) -> matplotlib 3.10 Colormap.__call__ (xa = x * N, xa == N -> N - 1,
// under / over / bad masks before the cast) -> (rgba[:3] * 255).astype(int), pre-multiplied into lut (N + 3 entries:
// 0..N-1, under, over, bad; r | g << 8 | b << 16)
__device__ __forceinline__ uint32_t obs_color(const double* xyzid, int mode, const double* stats, const uint32_t* lut,
                                              int N) {
  double t;
  if (mode == kPointOrder) {
    t = xyzid[3] / stats[5];
  } else {
    const double dx = xyzid[0] - stats[0], dy = xyzid[1] - stats[1], dz = xyzid[2] - stats[2];
    const double dis = sqrt((dx * dx + dy * dy) + dz * dz);
    t = (dis - stats[3]) / (stats[4] - stats[3]);
  }
  double xa = t * (double)N;
  if (xa == (double)N) xa = (double)(N - 1);
  int idx;
  if (xa != xa) idx = N + 2;
  else if (xa < 0.0) idx = N;
  else if (xa >= (double)N) idx = N + 1;
  else idx = (int)xa;
  return lut[idx];
}

// pass 1: centre (np.round: half to even), window test, colour; atomicMin of the depth key per cell
__global__ __launch_bounds__(256) void visible_min_kernel(const double* __restrict__ uvd, const double* __restrict__ xyzid,
                                                          const int64_t* __restrict__ obs_range, const int32_t* __restrict__ Hs,
                                                          const int32_t* __restrict__ Ws, const int64_t* __restrict__ grid_off,
                                                          int frame_begin, int r, int mode, const double* __restrict__ stats,
                                                          const uint32_t* __restrict__ lut, int N,
                                                          int32_t* __restrict__ obs_cell, uint32_t* __restrict__ color,
                                                          int32_t* __restrict__ centers,
                                                          unsigned long long* __restrict__ grid_key) {
  const FrameObs F = frame_obs(obs_range, Hs, Ws, grid_off, frame_begin, r);
  for (long o = F.a + blockIdx.x * (long)blockDim.x + threadIdx.x; o < F.b; o += (long)gridDim.x * blockDim.x) {
    const double cx = rint(uvd[3 * o]), cy = rint(uvd[3 * o + 1]);
    const double gx = cx + (double)r, gy = cy + (double)r;
    int cell = -1;
    if (gx >= 0.0 && gx < (double)F.gw && gy >= 0.0 && gy < (double)F.gh) {
      cell = (int)(F.base + (long)gy * F.gw + (long)gx);
      atomicMin(&grid_key[cell], depth_key(uvd[3 * o + 2]));
      if (centers) {
        centers[2 * o] = (int32_t)cx;
        centers[2 * o + 1] = (int32_t)cy;
      }
    } else if (centers) {
      centers[2 * o] = centers[2 * o + 1] = INT32_MIN;
    }
    obs_cell[o] = cell;
    if (lut) color[o] = obs_color(xyzid + 4 * o, mode, stats, lut, N);
  }
}

// pass 2: among the observations holding their cell's smallest key, the lowest index wins (np.argmin's first)
__global__ __launch_bounds__(256) void visible_idx_kernel(const double* __restrict__ uvd, const int64_t* __restrict__ obs_range,
                                                          const int32_t* __restrict__ Hs, const int32_t* __restrict__ Ws,
                                                          const int64_t* __restrict__ grid_off, int frame_begin, int r,
                                                          const int32_t* __restrict__ obs_cell,
                                                          const unsigned long long* __restrict__ grid_key,
                                                          uint32_t* __restrict__ grid_obs) {
  const FrameObs F = frame_obs(obs_range, Hs, Ws, grid_off, frame_begin, r);
  for (long o = F.a + blockIdx.x * (long)blockDim.x + threadIdx.x; o < F.b; o += (long)gridDim.x * blockDim.x) {
    const int cell = obs_cell[o];
    if (cell >= 0 && grid_key[cell] == depth_key(uvd[3 * o + 2])) atomicMin(&grid_obs[cell], (uint32_t)o);
  }
}

// pass 3 (optional): visible[o] = the observation is drawn
__global__ __launch_bounds__(256) void visible_mask_kernel(const int64_t* __restrict__ obs_range, const int32_t* __restrict__ Hs,
                                                           const int32_t* __restrict__ Ws, const int64_t* __restrict__ grid_off,
                                                           int frame_begin, int r, const int32_t* __restrict__ obs_cell,
                                                           const uint32_t* __restrict__ grid_obs, uint8_t* __restrict__ visible) {
  const FrameObs F = frame_obs(obs_range, Hs, Ws, grid_off, frame_begin, r);
  for (long o = F.a + blockIdx.x * (long)blockDim.x + threadIdx.x; o < F.b; o += (long)gridDim.x * blockDim.x) {
    const int cell = obs_cell[o];
    visible[o] = (cell >= 0 && grid_obs[cell] == (uint32_t)o) ? 1 : 0;
  }
}

// ------------------------------------------------------------------ compositing (utils.py:518-543)
// coverage of pixel (x, y) by the disc of radius r around (cx, cy), a = x - cx, b = y - cy: the number of the 4 x 4
// sub-samples at offsets (2i - 3) / 8 inside it; r = 0 covers its centre pixel fully
__device__ __forceinline__ int coverage(int a, int b, int r) {
  if (r == 0) return (a == 0 && b == 0) ? 16 : 0;
  const int R = 64 * r * r;
  int k = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int sx = 8 * a + 2 * i - 3;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int sy = 8 * b + 2 * j - 3;
      k += (sx * sx + sy * sy <= R) ? 1 : 0;
    }
  }
  return k;
}

// one thread per canvas pixel: zero in the pad, else the BGR source pixel with the winning circles within r blended in
// observation order (out = (old * (16 - k) + c * k + 8) >> 4).  The grid window around the tile is staged in LDS with a
// per-row occupancy bitmask, so that a pixel visits only the occupied cells of its (2r+1)^2 neighbourhood
__global__ __launch_bounds__(kTileW * kTileH) void draw_kernel(const uint8_t* __restrict__ images, const int64_t* __restrict__ img_off,
                                                               const int32_t* __restrict__ Hs, const int32_t* __restrict__ Ws,
                                                               const int64_t* __restrict__ grid_off, int frame_begin, int Hv,
                                                               int Wv, int r, const uint32_t* __restrict__ grid_obs,
                                                               const uint32_t* __restrict__ color, uint8_t* __restrict__ out) {
  extern __shared__ uint32_t lds[];
  const int side = 2 * r + 1, TW = kTileW + 2 * r, TH = kTileH + 2 * r, MW = (TW + 31) / 32;
  uint32_t* tile = lds;                       // TW x TH grid cells
  uint32_t* cov = tile + TW * TH;             // side x side coverage table
  uint32_t* occ = cov + side * side;          // TH x MW occupancy bits
  const int f = frame_begin + blockIdx.y;
  const int h = Hs[f], w = Ws[f];
  const int top = (Hv - h) / 2, left = (Wv - w) / 2;
  const int tiles_x = (Wv + kTileW - 1) / kTileW;
  const int X0 = (blockIdx.x % tiles_x) * kTileW, Y0 = (blockIdx.x / tiles_x) * kTileH;
  const int tx = threadIdx.x % kTileW, ty = threadIdx.x / kTileW;
  const int X = X0 + tx, Y = Y0 + ty;
  const int x0 = X0 - left, y0 = Y0 - top;     // image coordinates of the tile's corner
  const bool touches = x0 < w && x0 + kTileW > 0 && y0 < h && y0 + kTileH > 0;   // uniform over the block
  if (touches) {
    const int gw = w + 2 * r, gh = h + 2 * r;
    const uint32_t* g = grid_obs + (grid_off[f] - grid_off[frame_begin]);
    for (int i = threadIdx.x; i < TH * MW; i += blockDim.x) occ[i] = 0;
    for (int i = threadIdx.x; i < side * side; i += blockDim.x) cov[i] = coverage(r - i % side, r - i / side, r);
    __syncthreads();
    for (int i = threadIdx.x; i < TW * TH; i += blockDim.x) {
      const int col = i % TW, row = i / TW;
      const int gx = x0 + col, gy = y0 + row;   // window cell gx holds centre gx - r, i.e. pixel x's cells are x..x+2r
      const uint32_t o = (gx >= 0 && gx < gw && gy >= 0 && gy < gh) ? g[(long)gy * gw + gx] : kEmpty;
      tile[i] = o;
      if (o != kEmpty) atomicOr(&occ[row * MW + (col >> 5)], 1u << (col & 31));
    }
    __syncthreads();
  }
  if (X >= Wv || Y >= Hv) return;
  uint8_t* dst = out + (((size_t)blockIdx.y * Hv + Y) * Wv + X) * 3;
  const int x = X - left, y = Y - top;
  if (!(x >= 0 && x < w && y >= 0 && y < h)) {
    dst[0] = dst[1] = dst[2] = 0;
    return;
  }
  const uint8_t* src = images + img_off[f] + ((size_t)y * w + x) * 3;
  int c0 = src[2], c1 = src[1], c2 = src[0];     // RGB -> BGR
  const int cbeg = tx, cend = tx + side;         // this pixel's columns of the tile
  uint32_t lo = 0;
  for (;;) {                                     // next winner in observation order, until none is left
    uint32_t best = kEmpty;
    int bk = 0, left_over = 0;
    for (int dy = 0; dy < side; ++dy) {
      const uint32_t* mrow = occ + (ty + dy) * MW;
      const uint32_t* row = tile + (ty + dy) * TW;
      for (int wi = cbeg >> 5; wi <= (cend - 1) >> 5; ++wi) {
        const int base = wi << 5;
        uint32_t bits = mrow[wi];
        if (base < cbeg) bits &= ~0u << (cbeg - base);
        if (cend - base < 32) bits &= (1u << (cend - base)) - 1u;
        while (bits) {
          const int col = base + __ffs(bits) - 1;
          bits &= bits - 1u;
          const uint32_t o = row[col];
          if (o < lo) continue;
          const int k = (int)cov[dy * side + (col - tx)];
          if (!k) continue;
          ++left_over;
          if (o < best) {
            best = o;
            bk = k;
          }
        }
      }
    }
    if (best == kEmpty) break;
    const uint32_t c = color[best];
    c0 = (c0 * (16 - bk) + (int)(c & 255u) * bk + 8) >> 4;
    c1 = (c1 * (16 - bk) + (int)((c >> 8) & 255u) * bk + 8) >> 4;
    c2 = (c2 * (16 - bk) + (int)((c >> 16) & 255u) * bk + 8) >> 4;
    if (left_over == 1) break;                   // that was the last one
    lo = best + 1;
  }
  dst[0] = (uint8_t)c0;
  dst[1] = (uint8_t)c1;
  dst[2] = (uint8_t)c2;
}

dim3 obs_grid(long max_frame_obs, int frames) {
  return dim3((unsigned)std::max<long>(1, std::min<long>((max_frame_obs + 255) / 256, 1024)), (unsigned)frames);
}

}  // namespace
}  // namespace vgg

using namespace vgg;

extern "C" {

size_t vgg_reproj_stats_workspace_bytes(long num_points) {
  return (size_t)(kAccWords + 3 * std::max<long>(num_points, 0)) * sizeof(unsigned long long);
}

int vgg_reproj_stats(const double* xyz, const int64_t* point_id, long num_points, int color_mode, double* stats,
                     void* workspace, size_t workspace_bytes, void* stream) {
  if (num_points <= 0 || color_mode < 0 || color_mode > 2 || !stats) return VGG_ERR_INVALID_ARGUMENT;
  if ((color_mode != kPointOrder && !xyz) || (color_mode == kPointOrder && !point_id)) return VGG_ERR_INVALID_ARGUMENT;
  if (!workspace || workspace_bytes < vgg_reproj_stats_workspace_bytes(num_points)) return VGG_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* acc = (unsigned long long*)workspace;
  unsigned long long* keys = acc + kAccWords;
  const int grid = (int)std::min<long>((num_points + 255) / 256, 2048);
  if (color_mode == kDisToCenter) {
    stats_keys_kernel<<<grid, 256, 0, s>>>(xyz, num_points, keys, acc);
    VGG_LAUNCH_CHECK();
    stats_median_kernel<<<3, kStatsThreads, 0, s>>>(keys, num_points, acc, stats);
    VGG_LAUNCH_CHECK();
  } else {
    VGG_HIP_CHECK(hipMemsetAsync(stats, 0, 3 * sizeof(double), s));
    stats_keys_kernel<<<1, 256, 0, s>>>(xyz, 0, keys, acc);     // (accumulators only)
    VGG_LAUNCH_CHECK();
  }
  stats_dist_kernel<<<grid, 256, 0, s>>>(xyz, point_id, num_points, color_mode, stats, keys, acc);
  VGG_LAUNCH_CHECK();
  stats_final_kernel<<<1, kStatsThreads, 0, s>>>(keys, num_points, color_mode, acc, stats);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vgg_reproj_visible(const double* uvd, const double* xyzid, const int64_t* obs_range, const int32_t* heights,
                       const int32_t* widths, const int64_t* grid_off, int frame_begin, int frame_end, long max_frame_obs,
                       long chunk_cells, int draw_radius, int color_mode, const double* stats, const uint32_t* lut,
                       int lut_n, int32_t* obs_cell, uint32_t* color, int32_t* centers, uint8_t* visible,
                       unsigned long long* grid_key, uint32_t* grid_obs, void* stream) {
  if (frame_begin < 0 || frame_end < frame_begin || max_frame_obs < 0 || chunk_cells < 0 || draw_radius < 0 ||
      draw_radius > VGG_REPROJ_MAX_RADIUS)
    return VGG_ERR_INVALID_ARGUMENT;
  if (frame_end == frame_begin || chunk_cells == 0) return VGG_OK;
  if (!uvd || !obs_range || !heights || !widths || !grid_off || !obs_cell || !grid_key || !grid_obs)
    return VGG_ERR_INVALID_ARGUMENT;
  if (lut && (!xyzid || !stats || !color || lut_n <= 0 || color_mode < 0 || color_mode > 2)) return VGG_ERR_INVALID_ARGUMENT;
  if (chunk_cells > 0x7fffffffL || frame_end - frame_begin > 65535) return VGG_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  VGG_HIP_CHECK(hipMemsetAsync(grid_key, 0xff, (size_t)chunk_cells * sizeof(unsigned long long), s));
  VGG_HIP_CHECK(hipMemsetAsync(grid_obs, 0xff, (size_t)chunk_cells * sizeof(uint32_t), s));
  if (max_frame_obs == 0) return VGG_OK;                 // (the cleared grid: nothing is drawn)
  const dim3 grid = obs_grid(max_frame_obs, frame_end - frame_begin);
  visible_min_kernel<<<grid, 256, 0, s>>>(uvd, xyzid, obs_range, heights, widths, grid_off, frame_begin, draw_radius,
                                          color_mode, stats, lut, lut_n, obs_cell, color, centers, grid_key);
  VGG_LAUNCH_CHECK();
  visible_idx_kernel<<<grid, 256, 0, s>>>(uvd, obs_range, heights, widths, grid_off, frame_begin, draw_radius, obs_cell,
                                          grid_key, grid_obs);
  VGG_LAUNCH_CHECK();
  if (visible) {
    visible_mask_kernel<<<grid, 256, 0, s>>>(obs_range, heights, widths, grid_off, frame_begin, draw_radius, obs_cell,
                                             grid_obs, visible);
    VGG_LAUNCH_CHECK();
  }
  return VGG_OK;
}

int vgg_reproj_draw(const uint8_t* images, const int64_t* img_off, const int32_t* heights, const int32_t* widths,
                    const int64_t* grid_off, int frame_begin, int frame_end, int canvas_h, int canvas_w, int draw_radius,
                    const uint32_t* grid_obs, const uint32_t* color, uint8_t* out, void* stream) {
  if (frame_begin < 0 || frame_end < frame_begin || canvas_h < 0 || canvas_w < 0 || draw_radius < 0 ||
      draw_radius > VGG_REPROJ_MAX_RADIUS)
    return VGG_ERR_INVALID_ARGUMENT;
  if (frame_end == frame_begin || canvas_h == 0 || canvas_w == 0) return VGG_OK;
  if (!images || !img_off || !heights || !widths || !grid_off || !grid_obs || !color || !out) return VGG_ERR_INVALID_ARGUMENT;
  const long tiles = (long)((canvas_w + kTileW - 1) / kTileW) * ((canvas_h + kTileH - 1) / kTileH);
  if (tiles > 0x7fffffffL || frame_end - frame_begin > 65535) return VGG_ERR_UNSUPPORTED;
  const int side = 2 * draw_radius + 1;
  const int TW = kTileW + 2 * draw_radius, TH = kTileH + 2 * draw_radius;
  const size_t lds = (size_t)(TW * TH + side * side + TH * ((TW + 31) / 32)) * sizeof(uint32_t);
  draw_kernel<<<dim3((unsigned)tiles, (unsigned)(frame_end - frame_begin)), kTileW * kTileH, lds, (hipStream_t)stream>>>(
      images, img_off, heights, widths, grid_off, frame_begin, canvas_h, canvas_w, draw_radius, grid_obs, color, out);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

}  // extern "C"
