// The photometric matching cost of the dense stage: the staged reference tile, a lane's centred reference window and the
// cost nest, one copy for the plane sweep (mvs.hip) and the PatchMatch refinement (../patchmatch/patchmatch.hip).  Parity
// code: every sum in a stated order (tests/mvs_cases.py and tests/patchmatch_cases.py restate it in NumPy), and
// tests/test_gpu_patchmatch.py requires the two users to agree bit for bit on fronto-parallel planes.
#pragma once
#include <math.h>

#include "mvs_views.hpp"

namespace vgg {

// a TX x TY tile of reference pixels with its halo of R pixels, their rays, and per source its pose relative to the
// reference and its camera
template <int R, int TX, int TY>
struct CostTile {
  static constexpr int SX = TX + 2 * R, SY = TY + 2 * R, NPIX = SX * SY;
  float img[NPIX];
  double ray[NPIX][2];
  double rel[kMaxSources][12];
  double cam[kMaxSources][4];
};

// The tile, its halo and their rays, clamped to the frame (a lane past the frame's edge works on a copy of an edge pixel
// and only its store is guarded); lanes m < count derive the relative pose of source m.  Ends with a barrier.
template <int R, int TX, int TY>
__device__ __forceinline__ void cost_stage(CostTile<R, TX, TY>& t, const float* __restrict__ frames,
                                           const double* __restrict__ poses, const double* __restrict__ cams,
                                           const double* __restrict__ rays, int H, int W, const DenseViews& views) {
  constexpr int SX = CostTile<R, TX, TY>::SX, NPIX = CostTile<R, TX, TY>::NPIX;
  const int tid = threadIdx.x;
  const int tx0 = blockIdx.x * TX, ty0 = blockIdx.y * TY;
  const float* ref_img = frames + views.ref * ((long)H * W);
  for (int i = tid; i < NPIX; i += 256) {
    const int r = i / SX;
    const long p = (long)clampi(ty0 + r - R, H - 1) * W + clampi(tx0 + (i - r * SX) - R, W - 1);
    t.img[i] = ref_img[p];
    t.ray[i][0] = rays[2 * p];
    t.ray[i][1] = rays[2 * p + 1];
  }
  if (tid < views.count) {
    const int s = views.src[tid];
    relative_pose(poses + 12 * views.ref, poses + 12 * s, t.rel[tid]);
#pragma unroll
    for (int c = 0; c < 4; ++c) t.cam[tid][c] = cams[4 * s + c];
  }
  __syncthreads();
}

// a lane's pixel and its reference window, centred once
struct CostPixel {
  int x, y, centre;
  long pix;            // y W + x, clamped into the frame
  bool stored;
  double mA, sa, taa;
  bool textured;
};

// the pixel (lx, ly) of the tile, as the caller maps its lanes: mean, then the centred sums
template <int R, int TX, int TY>
__device__ __forceinline__ CostPixel cost_pixel(const CostTile<R, TX, TY>& t, int lx, int ly, int H, int W,
                                                double min_variance) {
  constexpr int SX = CostTile<R, TX, TY>::SX;
  constexpr double n = (double)((2 * R + 1) * (2 * R + 1));
  CostPixel p;
  p.x = blockIdx.x * TX + lx;
  p.y = blockIdx.y * TY + ly;
  p.centre = (ly + R) * SX + (lx + R);
  p.stored = p.x < W && p.y < H;
  p.pix = (long)min(p.y, H - 1) * W + min(p.x, W - 1);
  double sA = 0.0;
#pragma unroll
  for (int dy = -R; dy <= R; ++dy)
#pragma unroll
    for (int dx = -R; dx <= R; ++dx) sA += (double)t.img[p.centre + dy * SX + dx];
  p.mA = sA / n;
  double sa = 0.0, saa = 0.0;
#pragma unroll
  for (int dy = -R; dy <= R; ++dy)
#pragma unroll
    for (int dx = -R; dx <= R; ++dx) {
      const double a = (double)t.img[p.centre + dy * SX + dx] - p.mA;
      sa += a;
      saa += a * a;
    }
  p.sa = sa;
  p.taa = saa - sa * sa / n;
  p.textured = p.taa / n >= min_variance;
  return p;
}

// The inverse depth q of the window pixel with ray (u, v, 1), by value; false: the plane is behind that pixel.
struct FrontoParallel {   // one q for the window: always valid, no division per pixel
  double q;
  __device__ __forceinline__ bool operator()(double, double, double& qk) const {
    qk = q;
    return true;
  }
};
struct Slanted {          // 1 / w_k with w_k = (al u + be v) + ga
  double al, be, ga;
  __device__ __forceinline__ bool operator()(double u, double v, double& qk) const {
    const double wk = (al * u + be * v) + ga;
    qk = 1.0 / wk;
    return wk > 0.0;
  }
};

// The cost of a plane at the lane's pixel: sources outside, the window inside with its row loop rolled.  Validity is carried
// by selects.
template <int R, int TX, int TY, class InvDepth>
__device__ __forceinline__ double window_cost(const CostTile<R, TX, TY>& t, const CostPixel& p, const float* __restrict__ frames,
                                              const DenseViews& views, int H, int W, int min_views, const InvDepth inv_depth) {
  constexpr int SX = CostTile<R, TX, TY>::SX;
  constexpr double n = (double)((2 * R + 1) * (2 * R + 1));
  const long plane = (long)H * W;
  double acc = 0.0;
  int valid = 0;
  for (int m = 0; m < views.count; ++m) {
    const double* T = t.rel[m];
    const double* cam = t.cam[m];
    const float* img = frames + views.src[m] * plane;
    bool ok = true;
    double sb = 0.0, sbb = 0.0, sab = 0.0;
#pragma unroll 1
    for (int dy = -R; dy <= R; ++dy)
#pragma unroll
      for (int dx = -R; dx <= R; ++dx) {
        const int k = p.centre + dy * SX + dx;
        const double u = t.ray[k][0], v = t.ray[k][1];
        double q, xs, ys, zs;
        const bool before = inv_depth(u, v, q);
        const bool front = transfer_project(T, cam, u * q, v * q, q, xs, ys, zs);
        ok = ok && before && front && inside_image(xs, ys, H, W);
        const double a = (double)t.img[k] - p.mA;
        const double b = bilinear(img, H, W, xs, ys) - p.mA;
        sb += b;
        sbb += b * b;
        sab += a * b;
      }
    const double tbb = sbb - sb * sb / n, tab = sab - p.sa * sb / n;
    const double den = sqrt(p.taa * tbb);
    const double zncc = den > 0.0 ? tab / den : 0.0;
    acc = ok ? acc + (1.0 - zncc) : acc;
    valid += ok ? 1 : 0;
  }
  return (p.textured && valid >= min_views) ? acc / (double)valid : (double)INFINITY;
}

}  // namespace vgg
