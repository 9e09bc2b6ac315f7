// The pose, transfer and projection arithmetic that vggsfm_amd_mvs.h states under "Shared by both entries" and the sweep's
// bilinear sample: one copy, included (directly or through mvs_views.hpp and mvs_cost.hpp) by mvs.hip, ../fuse/fuse.hip,
// ../patchmatch/patchmatch.hip, ../tsdf/tsdf.hip, ../raster/raster.hip, ../klt/klt.hip and ../sim3.hip (all parity files,
// built with -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

namespace vgg {

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// [R|t] (3 x 4, row-major) of view b from view a
__device__ __forceinline__ void relative_pose(const double* __restrict__ pa, const double* __restrict__ pb, double* out) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) out[4 * i + j] = pb[4 * i] * pa[4 * j] + pb[4 * i + 1] * pa[4 * j + 1] + pb[4 * i + 2] * pa[4 * j + 2];
    out[4 * i + 3] = pb[4 * i + 3] - (out[4 * i] * pa[3] + out[4 * i + 1] * pa[7] + out[4 * i + 2] * pa[11]);
  }
}

// transfer P by T = [R|t]
__device__ __forceinline__ void transfer(const double* T, double p0, double p1, double p2, double& X0, double& X1, double& X2) {
  X0 = T[0] * p0 + T[1] * p1 + T[2] * p2 + T[3];
  X1 = T[4] * p0 + T[5] * p1 + T[6] * p2 + T[7];
  X2 = T[8] * p0 + T[9] * p1 + T[10] * p2 + T[11];
}

// the pixel of the normalised image point (a, b) under cam = f, cx, cy, k
__device__ __forceinline__ void project_normalised(const double* cam, double a, double b, double& x, double& y) {
  const double d = 1.0 + cam[3] * (a * a + b * b);
  x = cam[0] * (a * d) + cam[1];
  y = cam[0] * (b * d) + cam[2];
}

// transfer P by T = [R|t] and project with cam = f, cx, cy, k; false: behind the camera (x, y are then not to be used)
__device__ __forceinline__ bool transfer_project(const double* T, const double* cam, double p0, double p1, double p2, double& x,
                                                 double& y, double& z) {
  double X0, X1, X2;
  transfer(T, p0, p1, p2, X0, X1, X2);
  const double iz = 1.0 / X2;
  project_normalised(cam, X0 * iz, X1 * iz, x, y);
  z = X2;
  return X2 > 0.0;
}

// false for NaN and infinities too
__device__ __forceinline__ bool inside_image(double x, double y, int H, int W) {
  return x >= 0.0 && x <= (double)(W - 1) && y >= 0.0 && y <= (double)(H - 1);
}

// bilinear sample at (x, y); the coordinates are clamped to the image, so the loads stay in bounds whatever (x, y) is
// (a sample outside is computed and not used)
__device__ __forceinline__ double bilinear(const float* __restrict__ img, int H, int W, double x, double y) {
  x = fmin(fmax(x, 0.0), (double)(W - 1));
  y = fmin(fmax(y, 0.0), (double)(H - 1));
  const double xf = floor(x), yf = floor(y);
  const int x0 = (int)xf, y0 = (int)yf;
  const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
  const double fx = x - xf, fy = y - yf;
  const float* r0 = img + (long)y0 * W;
  const float* r1 = img + (long)y1 * W;
  const double i00 = (double)r0[x0], i01 = (double)r0[x1], i10 = (double)r1[x0], i11 = (double)r1[x1];
  return ((1.0 - fx) * (1.0 - fy)) * i00 + (fx * (1.0 - fy)) * i01 + ((1.0 - fx) * fy) * i10 + (fx * fy) * i11;
}

}  // namespace vgg
