// Plane-sweep multi-view stereo and the depth maps' consistency check for gfx950: the entries of vggsfm_amd_mvs.h.
// A parity file: built with -ffp-contract=off, every sum in a stated order (tests/mvs_cases.py restates it in NumPy).
#include <math.h>

#include "../common.hpp"
#include "mvs_geometry.hpp"
#include "vggsfm_amd_mvs.h"

namespace vgg {

constexpr int kTile = 16;                       // 16 x 16 reference pixels per workgroup, one wavefront per 16 x 4 block
constexpr int kMaxSources = VGGM_MAX_SOURCES;

// by-value kernel argument: the views of one call (validated on the host)
struct MvsViews {
  int32_t src[kMaxSources];
  int32_t src_ray[kMaxSources];
  int32_t ref, ref_ray, count;
};

// ------------------------------------------------------------------------------------------------------------ sweep
// One workgroup per 16 x 16 tile of reference pixels, one pixel per lane.  The tile with its halo of R pixels and the
// rays of those pixels are staged in LDS once (clamped to the image, so a lane past the image's edge works on a copy of
// an edge pixel and only its store is guarded); lanes m < count derive the relative pose of source m.  Then planes,
// sources, window: no cost volume is kept, a lane carries the previous plane's cost, the best cost and index and the
// costs before and after the best (the one after is captured on the next plane).  Validity is carried by selects.
template <int R>
__global__ __launch_bounds__(256) void mvs_sweep_kernel(const float* __restrict__ frames, const double* __restrict__ poses,
                                                       const double* __restrict__ cams, const double* __restrict__ rays, int H,
                                                       int W, MvsViews views, double w_far, double dw, int D, int min_views,
                                                       double min_variance, double min_conf, float* __restrict__ out_depth,
                                                       float* __restrict__ out_conf, int32_t* __restrict__ out_index,
                                                       double* __restrict__ out_cost) {
  constexpr int SIDE = kTile + 2 * R, NPIX = SIDE * SIDE;
  constexpr double n = (double)((2 * R + 1) * (2 * R + 1));
  __shared__ float s_img[NPIX];
  __shared__ double s_ray[NPIX][2];
  __shared__ double s_rel[kMaxSources][12];
  __shared__ double s_cam[kMaxSources][4];
  const int tid = threadIdx.x;
  const int tx0 = blockIdx.x * kTile, ty0 = blockIdx.y * kTile;
  const long plane = (long)H * W;
  const int M = views.count;
  {
    const float* ref_img = frames + views.ref * plane;
    for (int i = tid; i < NPIX; i += 256) {
      const int r = i / SIDE;
      const long p = (long)clampi(ty0 + r - R, H - 1) * W + clampi(tx0 + (i - r * SIDE) - R, W - 1);
      s_img[i] = ref_img[p];
      s_ray[i][0] = rays[2 * p];
      s_ray[i][1] = rays[2 * p + 1];
    }
    if (tid < M) {
      const int s = views.src[tid];
      relative_pose(poses + 12 * views.ref, poses + 12 * s, s_rel[tid]);
#pragma unroll
      for (int c = 0; c < 4; ++c) s_cam[tid][c] = cams[4 * s + c];
    }
  }
  __syncthreads();

  const int lx = tid & 15, ly = tid >> 4;
  const int centre = (ly + R) * SIDE + (lx + R);
  // the reference window: mean, then the centred sums
  double sA = 0.0;
#pragma unroll
  for (int dy = -R; dy <= R; ++dy)
#pragma unroll
    for (int dx = -R; dx <= R; ++dx) sA += (double)s_img[centre + dy * SIDE + dx];
  const double mA = sA / n;
  double sa = 0.0, saa = 0.0;
#pragma unroll
  for (int dy = -R; dy <= R; ++dy)
#pragma unroll
    for (int dx = -R; dx <= R; ++dx) {
      const double a = (double)s_img[centre + dy * SIDE + dx] - mA;
      sa += a;
      saa += a * a;
    }
  const double taa = saa - sa * sa / n;
  const bool textured = taa / n >= min_variance;

  const double inf = INFINITY;
  const int x = tx0 + lx, y = ty0 + ly;
  const bool stored = x < W && y < H;
  const long pix = (long)min(y, H - 1) * W + min(x, W - 1);
  double best = inf, c_prev = inf, c_minus = inf, c_plus = inf;
  int best_j = -1;
  for (int j = 0; j < D; ++j) {
    const double q = 1.0 / (w_far + (double)j * dw);
    double acc = 0.0;
    int valid = 0;
    for (int m = 0; m < M; ++m) {
      const double* T = s_rel[m];
      const double* cam = s_cam[m];
      const float* img = frames + views.src[m] * plane;
      bool ok = true;
      double sb = 0.0, sbb = 0.0, sab = 0.0;
#pragma unroll 1
      for (int dy = -R; dy <= R; ++dy)
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
          const int k = centre + dy * SIDE + dx;
          double xs, ys, zs;
          const bool front = transfer_project(T, cam, s_ray[k][0] * q, s_ray[k][1] * q, q, xs, ys, zs);
          ok = ok && front && inside_image(xs, ys, H, W);
          const double a = (double)s_img[k] - mA;
          const double b = bilinear(img, H, W, xs, ys) - mA;
          sb += b;
          sbb += b * b;
          sab += a * b;
        }
      const double tbb = sbb - sb * sb / n, tab = sab - sa * sb / n;
      const double den = sqrt(taa * tbb);
      const double zncc = den > 0.0 ? tab / den : 0.0;
      acc = ok ? acc + (1.0 - zncc) : acc;
      valid += ok ? 1 : 0;
    }
    const double cost = (textured && valid >= min_views) ? acc / (double)valid : inf;
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
// One lane per reference pixel; lanes m < count first derive both relative poses of source m.
__global__ __launch_bounds__(256) void mvs_filter_kernel(const float* __restrict__ depth, const double* __restrict__ poses,
                                                        const double* __restrict__ cams, const double* __restrict__ rays,
                                                        int H, int W, MvsViews views, double rel_depth_tol, double reproj_tol,
                                                        int min_consistent, float* __restrict__ out_depth,
                                                        int32_t* __restrict__ out_count) {
  __shared__ double s_fwd[kMaxSources][12];      // source from ref
  __shared__ double s_bwd[kMaxSources][12];      // ref from source
  __shared__ double s_cam[kMaxSources + 1][4];   // the sources', then ref's
  const int tid = threadIdx.x;
  const int M = views.count;
  if (tid < M) {
    const int s = views.src[tid];
    relative_pose(poses + 12 * views.ref, poses + 12 * s, s_fwd[tid]);
    relative_pose(poses + 12 * s, poses + 12 * views.ref, s_bwd[tid]);
#pragma unroll
    for (int c = 0; c < 4; ++c) s_cam[tid][c] = cams[4 * s + c];
  }
  if (tid < 4) s_cam[kMaxSources][tid] = cams[4 * views.ref + tid];
  __syncthreads();
  const long plane = (long)H * W;
  const long p = (long)blockIdx.x * 256 + tid;
  if (p >= plane) return;
  const int y = (int)(p / W), x = (int)(p - (long)y * W);
  const float zf = depth[views.ref * plane + p];
  const double z = (double)zf;
  int count = 0;
  if (z > 0.0) {
    const double* ray = rays + 2 * (views.ref_ray * plane + p);
    const double p0 = ray[0] * z, p1 = ray[1] * z;
    for (int m = 0; m < M; ++m) {
      double xs, ys, zc;
      if (!transfer_project(s_fwd[m], s_cam[m], p0, p1, z, xs, ys, zc)) continue;
      const double xi = floor(xs + 0.5), yi = floor(ys + 0.5);
      if (!inside_image(xi, yi, H, W)) continue;
      const long ps = (long)yi * W + (long)xi;
      const double zs = (double)depth[views.src[m] * plane + ps];
      if (!(zs > 0.0)) continue;
      const double* rs = rays + 2 * (views.src_ray[m] * plane + ps);
      double xb, yb, zb;
      if (!transfer_project(s_bwd[m], s_cam[kMaxSources], rs[0] * zs, rs[1] * zs, zs, xb, yb, zb)) continue;
      const double ex = xb - (double)x, ey = yb - (double)y;
      const bool near = sqrt(ex * ex + ey * ey) <= reproj_tol && fabs(zb - z) / z <= rel_depth_tol;
      count += near ? 1 : 0;
    }
  }
  out_count[p] = count;
  out_depth[p] = count >= min_consistent ? zf : 0.0f;
}

// the views of a call from its host arrays; false: refused
static bool make_views(int num_frames, int ref, const int32_t* sources, int num_sources, const int32_t* ray_index,
                       int num_rays, MvsViews* v) {
  if (num_frames < 1 || ref < 0 || ref >= num_frames || !sources || num_sources < 1 || num_sources > kMaxSources) return false;
  memset(v, 0, sizeof(*v));
  v->ref = ref;
  v->count = num_sources;
  for (int m = 0; m < num_sources; ++m) {
    if (sources[m] < 0 || sources[m] >= num_frames || sources[m] == ref) return false;
    v->src[m] = sources[m];
  }
  if (ray_index) {
    for (int s = 0; s < num_frames; ++s)
      if (ray_index[s] < 0 || ray_index[s] >= num_rays) return false;
    v->ref_ray = ray_index[ref];
    for (int m = 0; m < num_sources; ++m) v->src_ray[m] = ray_index[sources[m]];
  }
  return true;
}

}  // namespace vgg

using namespace vgg;

extern "C" {

const char* vggm_build_arch(void) { return "gfx950"; }

int vggm_plane_sweep(const float* frames, const double* poses, const double* cams, const double* rays, int num_frames,
                     int height, int width, int ref, const int32_t* sources, int num_sources, double inv_depth_far,
                     double inv_depth_near, int num_planes, int radius, int min_views, double min_variance, double min_conf,
                     float* out_depth, float* out_conf, int32_t* out_index, double* out_cost, void* stream) {
  MvsViews views;
  if (height < 0 || width < 0 || !make_views(num_frames, ref, sources, num_sources, nullptr, 0, &views))
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
  MvsViews views;
  if (height < 0 || width < 0 || num_rays < 1 || !ray_index ||
      !make_views(num_frames, ref, sources, num_sources, ray_index, num_rays, &views))
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
