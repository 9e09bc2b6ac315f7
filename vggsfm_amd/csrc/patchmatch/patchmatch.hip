// PatchMatch slanted-plane refinement of the multi-view stereo for gfx950: the entries of vggsfm_amd_patchmatch.h.
// A parity file: built with -ffp-contract=off, every sum in a stated order (tests/patchmatch_cases.py restates it in NumPy).
#include <math.h>

#include "../common.hpp"
#include "../mvs/mvs_cost.hpp"
#include "vggsfm_amd_patchmatch.h"

namespace vgg {

constexpr int kTileX = 32, kTileY = 16;         // 32 x 16 pixels per workgroup: 256 of each colour, one per lane
constexpr int kCandidates = 11;
static_assert(kMaxSources == VGGR_MAX_SOURCES, "mvs_views.hpp and vggsfm_amd_patchmatch.h disagree");

// what the cost needs besides the plane, by value
struct PmCost {
  int H, W, min_views;
  double min_variance;
};

__device__ __forceinline__ uint64_t pm_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ uint64_t pm_hash(uint64_t seed, uint64_t iteration, uint64_t colour, uint64_t pixel, uint64_t draw) {
  return pm_mix(pm_mix(pm_mix(pm_mix(pm_mix(seed + 0x9E3779B97F4A7C15ull) ^ iteration) ^ colour) ^ pixel) ^ draw);
}

__device__ __forceinline__ double pm_unit(uint64_t h) { return (double)(h >> 11) * 0x1p-53; }
__device__ __forceinline__ double pm_signed(uint64_t h) { return (double)(h >> 11) * 0x1p-52 - 1.0; }

// false for NaN
__device__ __forceinline__ bool pm_legal(double al, double be, double ga, double u0, double v0, double w_far, double w_near,
                                         double cos_tilt) {
  const double wc = (al * u0 + be * v0) + ga;
  return w_far <= wc && wc <= w_near &&
         wc * wc >= ((cos_tilt * cos_tilt) * ((al * al + be * be) + ga * ga)) * ((u0 * u0 + v0 * v0) + 1.0);
}

// The tile is staged and the cost stated by mvs_cost.hpp, as for the sweep, with one 1 / w_k per window pixel and source.
template <int R>
using PmTile = CostTile<R, kTileX, kTileY>;

// lane -> (2 i + parity(row, colour), row): the 256 pixels of one colour of the 32 x 16 tile
template <int R>
__device__ __forceinline__ CostPixel pm_pixel(const PmTile<R>& t, int colour, const PmCost& c) {
  const int ly = threadIdx.x >> 4, lx = 2 * (threadIdx.x & 15) + ((ly ^ colour) & 1);      // the tile's origin is even in x and y
  return cost_pixel(t, lx, ly, c.H, c.W, c.min_variance);
}

// -------------------------------------------------------------------------------------------------------------- cost
// One workgroup per 32 x 16 tile and colour (blockIdx.z): the cost of every pixel's own plane.
template <int R>
__global__ __launch_bounds__(256) void pm_cost_kernel(const float* __restrict__ frames, const double* __restrict__ poses,
                                                     const double* __restrict__ cams, const double* __restrict__ rays,
                                                     DenseViews views, PmCost c, const double* __restrict__ plane,
                                                     double* __restrict__ cost) {
  __shared__ PmTile<R> t;
  cost_stage(t, frames, poses, cams, rays, c.H, c.W, views);
  const CostPixel p = pm_pixel<R>(t, (int)blockIdx.z, c);
  const Slanted own = {plane[3 * p.pix], plane[3 * p.pix + 1], plane[3 * p.pix + 2]};
  const double value = window_cost(t, p, frames, views, c.H, c.W, c.min_views, own);
  if (p.stored) cost[p.pix] = value;
}

// -------------------------------------------------------------------------------------------------------------- step
// One workgroup per 32 x 16 tile, one ACTIVE pixel per lane.  A lane reads its own plane and cost and the planes of
// neighbours of the other colour, which this launch does not write; it writes its own plane and cost.  The candidate loop
// is rolled (one copy of the cost); a candidate that no lane of the wavefront may accept is skipped wave-uniformly.
struct PmStep {
  double w_far, w_near, depth_step, slope_step, cos_tilt, scale;
  unsigned long long seed;
  int iteration, colour;
};

template <int R>
__global__ __launch_bounds__(256) void pm_step_kernel(const float* __restrict__ frames, const double* __restrict__ poses,
                                                     const double* __restrict__ cams, const double* __restrict__ rays,
                                                     DenseViews views, PmCost c, PmStep s, double* plane, double* cost) {
  __shared__ PmTile<R> t;
  cost_stage(t, frames, poses, cams, rays, c.H, c.W, views);
  const CostPixel p = pm_pixel<R>(t, s.colour, c);
  const int H = c.H, W = c.W;
  const double u0 = t.ray[p.centre][0], v0 = t.ray[p.centre][1];
  double al = plane[3 * p.pix], be = plane[3 * p.pix + 1], ga = plane[3 * p.pix + 2];
  double best = cost[p.pix];
  const double r0 = pm_signed(pm_hash(s.seed, (uint64_t)s.iteration, (uint64_t)s.colour, (uint64_t)p.pix, 0));
  const double r1 = pm_signed(pm_hash(s.seed, (uint64_t)s.iteration, (uint64_t)s.colour, (uint64_t)p.pix, 1));
  const double r2 = pm_signed(pm_hash(s.seed, (uint64_t)s.iteration, (uint64_t)s.colour, (uint64_t)p.pix, 2));
  const double fa = (r0 * s.scale) * s.slope_step, fb = (r1 * s.scale) * s.slope_step, dw = (r2 * s.scale) * s.depth_step;
#pragma unroll 1
  for (int cand = 0; cand < kCandidates; ++cand) {
    double ca, cb, cg;
    bool use = p.stored;
    if (cand < 8) {                                     // kernel-uniform
      const int len = cand < 4 ? 1 : 3, sg = (cand & 1) ? len : -len;
      const int nx = p.x + ((cand & 2) ? 0 : sg), ny = p.y + ((cand & 2) ? sg : 0);
      use = use && nx >= 0 && nx < W && ny >= 0 && ny < H;
      const long q = (long)clampi(ny, H - 1) * W + clampi(nx, W - 1);
      ca = plane[3 * q];
      cb = plane[3 * q + 1];
      cg = plane[3 * q + 2];
    } else {
      const double wc = (al * u0 + be * v0) + ga;
      ca = cand != 9 ? al + fa * wc : al;
      cb = cand != 9 ? be + fb * wc : be;
      const double wn = cand != 10 ? wc + dw : wc;
      cg = wn - (ca * u0 + cb * v0);
    }
    const bool legal = use && pm_legal(ca, cb, cg, u0, v0, s.w_far, s.w_near, s.cos_tilt);
    if (__ballot(legal) == 0ull) continue;              // wave-uniform
    const double value = window_cost(t, p, frames, views, H, W, c.min_views, Slanted{ca, cb, cg});
    const bool better = legal && value < best;
    al = better ? ca : al;
    be = better ? cb : be;
    ga = better ? cg : ga;
    best = better ? value : best;
  }
  if (p.stored) {
    plane[3 * p.pix] = al;
    plane[3 * p.pix + 1] = be;
    plane[3 * p.pix + 2] = ga;
    cost[p.pix] = best;
  }
}

// ------------------------------------------------------------------------------------------------- init and outputs
// One lane per pixel.
__global__ __launch_bounds__(256) void pm_init_kernel(const float* __restrict__ depth, const float* __restrict__ normals,
                                                     const double* __restrict__ pose, const double* __restrict__ rays,
                                                     long count, double w_far, double w_near, double cos_tilt,
                                                     unsigned long long seed, double* __restrict__ plane) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= count) return;
  const double z = (double)depth[p];
  double al = 0.0, be = 0.0, ga;
  if (z > 0.0) {
    ga = 1.0 / z;
    if (normals != nullptr) {                           // kernel-uniform
      const double N0 = (double)normals[3 * p], N1 = (double)normals[3 * p + 1], N2 = (double)normals[3 * p + 2];
      const double u0 = rays[2 * p], v0 = rays[2 * p + 1];
      const double n0 = (pose[0] * N0 + pose[1] * N1) + pose[2] * N2;
      const double n1 = (pose[4] * N0 + pose[5] * N1) + pose[6] * N2;
      const double n2 = (pose[8] * N0 + pose[9] * N1) + pose[10] * N2;
      const double d = ((n0 * u0 + n1 * v0) + n2) * z;
      const double pa = n0 / d, pb = n1 / d, pg = n2 / d;
      const bool take = (N0 != 0.0 || N1 != 0.0 || N2 != 0.0) && pm_legal(pa, pb, pg, u0, v0, w_far, w_near, cos_tilt);
      al = take ? pa : al;
      be = take ? pb : be;
      ga = take ? pg : ga;
    }
  } else {
    ga = w_far + pm_unit(pm_hash(seed, ~0ull, 0, (uint64_t)p, 0)) * (w_near - w_far);
  }
  plane[3 * p] = al;
  plane[3 * p + 1] = be;
  plane[3 * p + 2] = ga;
}

__global__ __launch_bounds__(256) void pm_outputs_kernel(const double* __restrict__ plane, const double* __restrict__ cost,
                                                        const double* __restrict__ pose, const double* __restrict__ rays,
                                                        long count, double min_conf, float* __restrict__ out_depth,
                                                        float* __restrict__ out_conf, float* __restrict__ out_normal) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= count) return;
  const double al = plane[3 * p], be = plane[3 * p + 1], ga = plane[3 * p + 2], c = cost[p];
  const double wc = (al * rays[2 * p] + be * rays[2 * p + 1]) + ga;
  const bool found = isfinite(c);
  const double conf = found ? 1.0 - c : 0.0;
  const bool keep = found && wc > 0.0 && !(conf < min_conf);
  double m[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) m[i] = -((pose[i] * al + pose[4 + i] * be) + pose[8 + i] * ga);
  const double l = sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
  out_depth[p] = keep ? (float)(1.0 / wc) : 0.0f;
  out_conf[p] = (float)conf;
#pragma unroll
  for (int i = 0; i < 3; ++i) out_normal[3 * p + i] = (keep && l > 0.0) ? (float)(m[i] / l) : 0.0f;
}

// ---------------------------------------------------------------------------------------------------- host checks
static bool frame_ok(int num_frames, int height, int width, int ref) {
  return num_frames >= 1 && height >= 0 && width >= 0 && ref >= 0 && ref < num_frames;
}

static bool range_ok(double w_far, double w_near, double cos_tilt) {
  return w_far > 0.0 && w_far < w_near && isfinite(w_near) && cos_tilt >= 0.0 && cos_tilt <= 1.0;
}

// the views of a call and the window's limits; false: refused
static bool window_ok(int num_frames, int ref, const int32_t* sources, int num_sources, int radius, int min_views,
                      DenseViews* v) {
  return make_views(num_frames, ref, sources, num_sources, 1, nullptr, 0, v) && radius >= 1 && radius <= VGGR_MAX_RADIUS &&
         min_views >= 1 && min_views <= num_sources;
}

static bool size_ok(int height, int width) {
  return (long)height * width <= (long)INT32_MAX && div_up(height, kTileY) <= 65535;
}

}  // namespace vgg

using namespace vgg;

extern "C" {

const char* vggr_build_arch(void) { return "gfx950"; }

int vggr_plane_init(const float* depth, const float* normals, const double* poses, const double* rays, int num_frames,
                    int height, int width, int ref, double inv_depth_far, double inv_depth_near, double cos_max_tilt,
                    unsigned long long seed, double* plane, void* stream) {
  if (!frame_ok(num_frames, height, width, ref) || !range_ok(inv_depth_far, inv_depth_near, cos_max_tilt))
    return VGG_ERR_INVALID_ARGUMENT;
  if (height == 0 || width == 0) return VGG_OK;
  if (!depth || !poses || !rays || !plane) return VGG_ERR_INVALID_ARGUMENT;
  if (!size_ok(height, width)) return VGG_ERR_UNSUPPORTED;
  const long count = (long)height * width;
  pm_init_kernel<<<div_up(count, 256), 256, 0, (hipStream_t)stream>>>(depth, normals, poses + 12 * ref, rays, count,
                                                                      inv_depth_far, inv_depth_near, cos_max_tilt, seed, plane);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vggr_plane_cost(const float* frames, const double* poses, const double* cams, const double* rays, int num_frames,
                    int height, int width, int ref, const int32_t* sources, int num_sources, int radius, int min_views,
                    double min_variance, const double* plane, double* cost, void* stream) {
  DenseViews views;
  if (!frame_ok(num_frames, height, width, ref) || !window_ok(num_frames, ref, sources, num_sources, radius, min_views, &views))
    return VGG_ERR_INVALID_ARGUMENT;
  if (height == 0 || width == 0) return VGG_OK;
  if (!frames || !poses || !cams || !rays || !plane || !cost) return VGG_ERR_INVALID_ARGUMENT;
  if (!size_ok(height, width)) return VGG_ERR_UNSUPPORTED;
  const PmCost c = {height, width, min_views, min_variance};
  const dim3 grid(div_up(width, kTileX), div_up(height, kTileY), 2);
  hipStream_t st = (hipStream_t)stream;
  if (radius == 1) pm_cost_kernel<1><<<grid, 256, 0, st>>>(frames, poses, cams, rays, views, c, plane, cost);
  else if (radius == 2) pm_cost_kernel<2><<<grid, 256, 0, st>>>(frames, poses, cams, rays, views, c, plane, cost);
  else pm_cost_kernel<3><<<grid, 256, 0, st>>>(frames, poses, cams, rays, views, c, plane, cost);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vggr_step(const float* frames, const double* poses, const double* cams, const double* rays, int num_frames, int height,
              int width, int ref, const int32_t* sources, int num_sources, int radius, int min_views, double min_variance,
              double inv_depth_far, double inv_depth_near, double depth_step, double slope_step, double cos_max_tilt,
              unsigned long long seed, int iteration, int colour, double* plane, double* cost, void* stream) {
  DenseViews views;
  if (!frame_ok(num_frames, height, width, ref) || !window_ok(num_frames, ref, sources, num_sources, radius, min_views, &views) ||
      !range_ok(inv_depth_far, inv_depth_near, cos_max_tilt))
    return VGG_ERR_INVALID_ARGUMENT;
  if (colour < 0 || colour > 1 || iteration < 0 || !(depth_step >= 0.0) || !(slope_step >= 0.0) || !isfinite(depth_step) ||
      !isfinite(slope_step))
    return VGG_ERR_INVALID_ARGUMENT;
  if (height == 0 || width == 0) return VGG_OK;
  if (!frames || !poses || !cams || !rays || !plane || !cost) return VGG_ERR_INVALID_ARGUMENT;
  if (!size_ok(height, width)) return VGG_ERR_UNSUPPORTED;
  const PmCost c = {height, width, min_views, min_variance};
  const PmStep s = {inv_depth_far, inv_depth_near, depth_step, slope_step, cos_max_tilt, ldexp(1.0, -iteration), seed,
                    iteration,     colour};
  const dim3 grid(div_up(width, kTileX), div_up(height, kTileY));
  hipStream_t st = (hipStream_t)stream;
  if (radius == 1) pm_step_kernel<1><<<grid, 256, 0, st>>>(frames, poses, cams, rays, views, c, s, plane, cost);
  else if (radius == 2) pm_step_kernel<2><<<grid, 256, 0, st>>>(frames, poses, cams, rays, views, c, s, plane, cost);
  else pm_step_kernel<3><<<grid, 256, 0, st>>>(frames, poses, cams, rays, views, c, s, plane, cost);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vggr_outputs(const double* plane, const double* cost, const double* poses, const double* rays, int num_frames, int height,
                 int width, int ref, double min_conf, float* out_depth, float* out_conf, float* out_normal, void* stream) {
  if (!frame_ok(num_frames, height, width, ref) || min_conf != min_conf) return VGG_ERR_INVALID_ARGUMENT;
  if (height == 0 || width == 0) return VGG_OK;
  if (!plane || !cost || !poses || !rays || !out_depth || !out_conf || !out_normal) return VGG_ERR_INVALID_ARGUMENT;
  if (!size_ok(height, width)) return VGG_ERR_UNSUPPORTED;
  const long count = (long)height * width;
  pm_outputs_kernel<<<div_up(count, 256), 256, 0, (hipStream_t)stream>>>(plane, cost, poses + 12 * ref, rays, count, min_conf,
                                                                         out_depth, out_conf, out_normal);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

}  // extern "C"
