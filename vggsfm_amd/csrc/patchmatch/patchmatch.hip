// PatchMatch slanted-plane refinement of the multi-view stereo for gfx950: the entries of vggsfm_amd_patchmatch.h.
// A parity file: built with -ffp-contract=off, every sum in a stated order (tests/patchmatch_cases.py restates it in NumPy).
#include <math.h>

#include "../common.hpp"
#include "../mvs/mvs_geometry.hpp"
#include "vggsfm_amd_patchmatch.h"

namespace vgg {

constexpr int kTileX = 32, kTileY = 16;         // 32 x 16 pixels per workgroup: 256 of each colour, one per lane
constexpr int kMaxSources = VGGR_MAX_SOURCES;
constexpr int kCandidates = 11;

// by-value kernel argument: the views of one call (validated on the host)
struct PmViews {
  int32_t src[kMaxSources];
  int32_t ref, count;
};

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

template <int R>
struct PmTile {
  static constexpr int SX = kTileX + 2 * R, SY = kTileY + 2 * R, NPIX = SX * SY;
  float img[NPIX];
  double ray[NPIX][2];
  double rel[kMaxSources][12];
  double cam[kMaxSources][4];
};

// The tile, its halo of R pixels and their rays, clamped to the frame as the sweep stages them (a lane past the frame's
// edge works on a copy of an edge pixel and stores nothing); lanes m < count derive the relative pose of source m.
// Ends with the kernels' only barrier.
template <int R>
__device__ __forceinline__ void pm_stage(PmTile<R>& t, const float* __restrict__ frames, const double* __restrict__ poses,
                                         const double* __restrict__ cams, const double* __restrict__ rays, int H, int W,
                                         const PmViews& views) {
  constexpr int SX = PmTile<R>::SX, NPIX = PmTile<R>::NPIX;
  const int tid = threadIdx.x;
  const int tx0 = blockIdx.x * kTileX, ty0 = blockIdx.y * kTileY;
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
struct PmPixel {
  int x, y, centre;
  long pix;            // y W + x, clamped into the frame
  bool stored;
  double mA, sa, taa;
  bool textured;
};

// lane -> (2 i + parity(row, colour), row): the 256 pixels of one colour of the 32 x 16 tile
template <int R>
__device__ __forceinline__ PmPixel pm_pixel(const PmTile<R>& t, int colour, int H, int W, double min_variance) {
  constexpr int SX = PmTile<R>::SX;
  constexpr double n = (double)((2 * R + 1) * (2 * R + 1));
  const int tid = threadIdx.x;
  const int ly = tid >> 4, lx = 2 * (tid & 15) + ((ly ^ colour) & 1);      // the tile's origin is even in x and y
  PmPixel p;
  p.x = blockIdx.x * kTileX + lx;
  p.y = blockIdx.y * kTileY + ly;
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

// The cost of plane (al, be, ga) at the lane's pixel: the sweep's nest (sources outside, the window inside with its row
// loop rolled), one 1 / w_k per window pixel and source.  Validity is carried by selects.
template <int R>
__device__ __forceinline__ double pm_cost(const PmTile<R>& t, const PmPixel& p, const float* __restrict__ frames,
                                          const PmViews& views, const PmCost& c, double al, double be, double ga) {
  constexpr int SX = PmTile<R>::SX;
  constexpr double n = (double)((2 * R + 1) * (2 * R + 1));
  const long plane = (long)c.H * c.W;
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
        const double wk = (al * u + be * v) + ga;
        const double q = 1.0 / wk;
        double xs, ys, zs;
        const bool front = transfer_project(T, cam, u * q, v * q, q, xs, ys, zs);
        ok = ok && wk > 0.0 && front && inside_image(xs, ys, c.H, c.W);
        const double a = (double)t.img[k] - p.mA;
        const double b = bilinear(img, c.H, c.W, xs, ys) - p.mA;
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
  return (p.textured && valid >= c.min_views) ? acc / (double)valid : (double)INFINITY;
}

// -------------------------------------------------------------------------------------------------------------- cost
// One workgroup per 32 x 16 tile and colour (blockIdx.z): the cost of every pixel's own plane.
template <int R>
__global__ __launch_bounds__(256) void pm_cost_kernel(const float* __restrict__ frames, const double* __restrict__ poses,
                                                     const double* __restrict__ cams, const double* __restrict__ rays,
                                                     PmViews views, PmCost c, const double* __restrict__ plane,
                                                     double* __restrict__ cost) {
  __shared__ PmTile<R> t;
  pm_stage<R>(t, frames, poses, cams, rays, c.H, c.W, views);
  const PmPixel p = pm_pixel<R>(t, (int)blockIdx.z, c.H, c.W, c.min_variance);
  const double value = pm_cost<R>(t, p, frames, views, c, plane[3 * p.pix], plane[3 * p.pix + 1], plane[3 * p.pix + 2]);
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
                                                     PmViews views, PmCost c, PmStep s, double* plane, double* cost) {
  __shared__ PmTile<R> t;
  pm_stage<R>(t, frames, poses, cams, rays, c.H, c.W, views);
  const PmPixel p = pm_pixel<R>(t, s.colour, c.H, c.W, c.min_variance);
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
    const double value = pm_cost<R>(t, p, frames, views, c, ca, cb, cg);
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

// the views of a call from its host array; false: refused
static bool make_views(int num_frames, int ref, const int32_t* sources, int num_sources, int radius, int min_views, PmViews* v) {
  if (!sources || num_sources < 1 || num_sources > kMaxSources || radius < 1 || radius > VGGR_MAX_RADIUS || min_views < 1 ||
      min_views > num_sources)
    return false;
  memset(v, 0, sizeof(*v));
  v->ref = ref;
  v->count = num_sources;
  for (int m = 0; m < num_sources; ++m) {
    if (sources[m] < 0 || sources[m] >= num_frames || sources[m] == ref) return false;
    v->src[m] = sources[m];
  }
  return true;
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
  PmViews views;
  if (!frame_ok(num_frames, height, width, ref) || !make_views(num_frames, ref, sources, num_sources, radius, min_views, &views))
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
  PmViews views;
  if (!frame_ok(num_frames, height, width, ref) || !make_views(num_frames, ref, sources, num_sources, radius, min_views, &views) ||
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
