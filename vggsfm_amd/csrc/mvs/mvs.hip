// Plane-sweep multi-view stereo and the depth maps' consistency check for gfx950: the entries of vggsfm_amd_mvs.h.
// A parity file: built with -ffp-contract=off, every sum in a stated order (tests/mvs_cases.py restates it in NumPy).
#include <math.h>

#include "../common.hpp"
#include "mvs_cost.hpp"
#include "vggsfm_amd_mvs.h"

namespace vgg {

constexpr int kTile = 16;                       // 16 x 16 reference pixels per workgroup, one wavefront per 16 x 4 block
static_assert(kMaxSources == VGGM_MAX_SOURCES, "mvs_views.hpp and vggsfm_amd_mvs.h disagree");

// ------------------------------------------------------------------------------------------------------------ sweep
// One workgroup per 16 x 16 tile of reference pixels, one pixel per lane, row-major (mvs_cost.hpp stages the tile and
// states the cost).  Planes outside, one 1 / w per plane: no cost volume is kept, a lane carries the previous plane's cost,
// the best cost and index and the costs before and after the best (the one after is captured on the next plane).
template <int R>
__global__ __launch_bounds__(256) void mvs_sweep_kernel(const float* __restrict__ frames, const double* __restrict__ poses,
                                                       const double* __restrict__ cams, const double* __restrict__ rays, int H,
                                                       int W, DenseViews views, double w_far, double dw, int D, int min_views,
                                                       double min_variance, double min_conf, float* __restrict__ out_depth,
                                                       float* __restrict__ out_conf, int32_t* __restrict__ out_index,
                                                       double* __restrict__ out_cost) {
  __shared__ CostTile<R, kTile, kTile> t;
  cost_stage(t, frames, poses, cams, rays, H, W, views);
  const CostPixel p = cost_pixel(t, (int)threadIdx.x & 15, (int)threadIdx.x >> 4, H, W, min_variance);
  const double inf = INFINITY;
  const long plane = (long)H * W, pix = p.pix;
  const bool stored = p.stored;
  double best = inf, c_prev = inf, c_minus = inf, c_plus = inf;
  int best_j = -1;
  for (int j = 0; j < D; ++j) {
    const double cost = window_cost(t, p, frames, views, H, W, min_views, FrontoParallel{1.0 / (w_far + (double)j * dw)});
    if (out_cost != nullptr) {                       // kernel-uniform
      if (stored) out_cost[(long)j * plane + pix] = cost;
    }
    c_plus = (best_j >= 0 && best_j == j - 1) ? cost : c_plus;
    const bool better = cost < best;
    c_minus = better ? c_prev : c_minus;
    c_plus = better ? inf : c_plus;
    best_j = better ? j : best_j;
    best = better ? cost : best;
    c_prev = cost;
  }

  const bool found = best_j >= 0;
  const double conf = found ? 1.0 - best : 0.0;
  double w = w_far + (double)(found ? best_j : 0) * dw;
  const double e = c_minus - 2.0 * best + c_plus;
  const bool refine = best_j > 0 && best_j < D - 1 && isfinite(c_minus) && isfinite(c_plus) && e > 0.0;
  w = refine ? w + ((0.5 * (c_minus - c_plus)) / e) * dw : w;
  const bool keep = found && !(conf < min_conf);
  if (stored) {
    out_depth[pix] = keep ? (float)(1.0 / w) : 0.0f;
    out_conf[pix] = (float)conf;
    out_index[pix] = keep ? best_j : -1;
  }
}

// ------------------------------------------------------------------------------------------------------------ filter
// One lane per reference pixel, counting the sources that confirm it (mvs_views.hpp).
__global__ __launch_bounds__(256) void mvs_filter_kernel(const float* __restrict__ depth, const double* __restrict__ poses,
                                                        const double* __restrict__ cams, const double* __restrict__ rays,
                                                        int H, int W, DenseViews views, double rel_depth_tol, double reproj_tol,
                                                        int min_consistent, float* __restrict__ out_depth,
                                                        int32_t* __restrict__ out_count) {
  __shared__ ViewPoses s;
  stage_view_poses(s, poses, cams, views);
  __syncthreads();
  const long plane = (long)H * W;
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= plane) return;
  const int y = (int)(p / W), x = (int)(p - (long)y * W);
  const float zf = depth[views.ref * plane + p];
  const double z = (double)zf;
  int count = 0;
  if (z > 0.0) {
    const double* ray = rays + 2 * (views.ref_ray * plane + p);
    const double p0 = ray[0] * z, p1 = ray[1] * z;
    for (int m = 0; m < views.count; ++m) {
      SourceHit hit;
      count += source_confirms(s, views, m, depth, rays, H, W, x, y, p0, p1, z, reproj_tol, rel_depth_tol, hit) ? 1 : 0;
    }
  }
  out_count[p] = count;
  out_depth[p] = count >= min_consistent ? zf : 0.0f;
}

}  // namespace vgg

using namespace vgg;

extern "C" {

const char* vggm_build_arch(void) { return "gfx950"; }

int vggm_plane_sweep(const float* frames, const double* poses, const double* cams, const double* rays, int num_frames,
                     int height, int width, int ref, const int32_t* sources, int num_sources, double inv_depth_far,
                     double inv_depth_near, int num_planes, int radius, int min_views, double min_variance, double min_conf,
                     float* out_depth, float* out_conf, int32_t* out_index, double* out_cost, void* stream) {
  DenseViews views;
  if (height < 0 || width < 0 || !make_views(num_frames, ref, sources, num_sources, 1, nullptr, 0, &views))
    return VGG_ERR_INVALID_ARGUMENT;
  if (num_planes < 1 || num_planes > VGGM_MAX_PLANES || radius < 1 || radius > VGGM_MAX_RADIUS || min_views < 1 ||
      min_views > num_sources)
    return VGG_ERR_INVALID_ARGUMENT;
  if (!(inv_depth_far > 0.0 && inv_depth_far < inv_depth_near && isfinite(inv_depth_near))) return VGG_ERR_INVALID_ARGUMENT;
  if (height == 0 || width == 0) return VGG_OK;
  if (!frames || !poses || !cams || !rays || !out_depth || !out_conf || !out_index) return VGG_ERR_INVALID_ARGUMENT;
  const long plane = (long)height * width;
  if (plane > (long)INT32_MAX || div_up(height, kTile) > 65535) return VGG_ERR_UNSUPPORTED;
  const double dw = num_planes > 1 ? (inv_depth_near - inv_depth_far) / (double)(num_planes - 1) : 0.0;
  const dim3 grid(div_up(width, kTile), div_up(height, kTile));
  hipStream_t st = (hipStream_t)stream;
#define VGGM_SWEEP(R)                                                                                                     \
  mvs_sweep_kernel<R><<<grid, 256, 0, st>>>(frames, poses, cams, rays, height, width, views, inv_depth_far, dw, num_planes, \
                                            min_views, min_variance, min_conf, out_depth, out_conf, out_index, out_cost)
  if (radius == 1) VGGM_SWEEP(1);
  else if (radius == 2) VGGM_SWEEP(2);
  else VGGM_SWEEP(3);
#undef VGGM_SWEEP
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vggm_consistency_filter(const float* depth, const double* poses, const double* cams, const double* rays,
                            const int32_t* ray_index, int num_rays, int num_frames, int height, int width, int ref,
                            const int32_t* sources, int num_sources, double rel_depth_tol, double reproj_tol,
                            int min_consistent, float* out_depth, int32_t* out_count, void* stream) {
  DenseViews views;
  if (height < 0 || width < 0 || num_rays < 1 || !ray_index ||
      !make_views(num_frames, ref, sources, num_sources, 1, ray_index, num_rays, &views))
    return VGG_ERR_INVALID_ARGUMENT;
  if (min_consistent < 1 || !(rel_depth_tol >= 0.0) || !(reproj_tol >= 0.0)) return VGG_ERR_INVALID_ARGUMENT;
  if (height == 0 || width == 0) return VGG_OK;
  if (!depth || !poses || !cams || !rays || !out_depth || !out_count) return VGG_ERR_INVALID_ARGUMENT;
  const long plane = (long)height * width;
  if (plane > (long)INT32_MAX) return VGG_ERR_UNSUPPORTED;
  mvs_filter_kernel<<<div_up(plane, 256), 256, 0, (hipStream_t)stream>>>(depth, poses, cams, rays, height, width, views,
                                                                         rel_depth_tol, reproj_tol, min_consistent,
                                                                         out_depth, out_count);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

}  // extern "C"
