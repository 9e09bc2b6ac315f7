// Fusion of the depth maps into one point cloud for gfx950: the entries of vggsfm_amd_fuse.h.
// A parity file: built with -ffp-contract=off, every sum in a stated order (tests/fusion_cases.py restates it in NumPy).
#include <math.h>

#include "../common.hpp"
#include "../scan.hpp"
#include "../mvs/mvs_views.hpp"
#include "vggsfm_amd_fuse.h"

namespace vgg {

constexpr int kTile = 16;                       // normals: 16 x 16 pixels per workgroup, staged with a halo of 1
static_assert(kMaxSources == VGGF_MAX_SOURCES, "mvs_views.hpp and vggsfm_amd_fuse.h disagree");
constexpr int kNormalViews = 256;               // views per launch of the normals kernel
constexpr int kFuseThreads = 256, kFuseWaves = kFuseThreads / kWave;

// by-value kernel argument, validated on the host
struct NormalViews {
  int32_t first;
  int32_t ray[kNormalViews];
};

// ----------------------------------------------------------------------------------------------------------- normals
// One workgroup per 16 x 16 tile of one view (blockIdx.z), one pixel per lane.  The camera-frame points of the tile and
// of its halo of 1 are staged in LDS once; a halo pixel outside the frame is staged with z = 0, so it never counts (its
// loads are clamped to the frame).  A lane past the frame's edge works on such a pixel and only its store is guarded.
__global__ __launch_bounds__(256) void fuse_normals_kernel(const float* __restrict__ depth, const double* __restrict__ poses,
                                                          const double* __restrict__ rays, int H, int W, NormalViews views,
                                                          double max_rel_jump, float* __restrict__ out) {
  constexpr int SIDE = kTile + 2, NPIX = SIDE * SIDE;
  __shared__ double s_p[NPIX][3];
  const int tid = threadIdx.x;
  const int tx0 = blockIdx.x * kTile, ty0 = blockIdx.y * kTile;
  const long plane = (long)H * W;
  const long s = (long)views.first + blockIdx.z;
  const float* dm = depth + s * plane;
  const double* rm = rays + 2 * ((long)views.ray[blockIdx.z] * plane);
  for (int i = tid; i < NPIX; i += 256) {
    const int r = i / SIDE;
    const int yy = ty0 + r - 1, xx = tx0 + (i - r * SIDE) - 1;
    const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
    const long p = (long)clampi(yy, H - 1) * W + clampi(xx, W - 1);
    const double z = in ? (double)dm[p] : 0.0;
    s_p[i][0] = rm[2 * p] * z;
    s_p[i][1] = rm[2 * p + 1] * z;
    s_p[i][2] = z;
  }
  __syncthreads();

  const int lx = tid & 15, ly = tid >> 4;
  const int c = (ly + 1) * SIDE + (lx + 1);
  const int x = tx0 + lx, y = ty0 + ly;
  const double P0 = s_p[c][0], P1 = s_p[c][1], z = s_p[c][2];
  const double jump = max_rel_jump * z;
  bool has = z > 0.0;
  double g[2][3];
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int step = a == 0 ? 1 : SIDE;
    const int kp = c + step, km = c - step;
    const double zp = s_p[kp][2], zm = s_p[km][2];
    const bool plus = zp > 0.0 && fabs(zp - z) <= jump, minus = zm > 0.0 && fabs(zm - z) <= jump;
    has = has && (plus || minus);
    const int hi = plus ? kp : c, lo = minus ? km : c;
#pragma unroll
    for (int i = 0; i < 3; ++i) g[a][i] = s_p[hi][i] - s_p[lo][i];
  }
  const double n0 = g[0][1] * g[1][2] - g[0][2] * g[1][1];
  const double n1 = g[0][2] * g[1][0] - g[0][0] * g[1][2];
  const double n2 = g[0][0] * g[1][1] - g[0][1] * g[1][0];
  const double len = sqrt(n0 * n0 + n1 * n1 + n2 * n2);
  const double d = n0 * P0 + n1 * P1 + n2 * z;
  has = has && len > 0.0 && (d < 0.0 || d > 0.0);
  double m0 = n0 / len, m1 = n1 / len, m2 = n2 / len;
  if (d > 0.0) { m0 = -m0; m1 = -m1; m2 = -m2; }
  if (x < W && y < H) {
    const double* R = poses + 12 * s;
    float* o = out + 3 * (s * plane + (long)y * W + x);
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = has ? (float)(R[i] * m0 + R[4 + i] * m1 + R[8 + i] * m2) : 0.0f;
  }
}

// ------------------------------------------------------------------------------------------------------------ fusion
// One lane per pixel of the view (views.ref); the poses are staged and a source's confirmation is tested as in
// mvs_filter_kernel (mvs_views.hpp), and lanes m <= count copy the poses themselves.  Every pixel writes stage_views
// (0: no point), a pixel that emits its staged point and its claims; the workgroup writes its number of points.
__global__ __launch_bounds__(kFuseThreads) void fuse_view_kernel(
    const float* __restrict__ depth, const float* __restrict__ normals, const float* __restrict__ frames,
    const double* __restrict__ poses, const double* __restrict__ cams, const double* __restrict__ rays, int H, int W,
    DenseViews views, double rel_depth_tol, double reproj_tol, double min_normal_cos, int min_views, uint8_t* claimed,
    int32_t* __restrict__ stage_views, double* __restrict__ stage_xyz, float* __restrict__ stage_normal,
    float* __restrict__ stage_rgb, int32_t* __restrict__ block_counts) {
  __shared__ ViewPoses s_rel;
  __shared__ double s_pose[kMaxSources + 1][12]; // the sources', then the view's
  __shared__ int s_pix[kMaxSources][kFuseThreads];   // per lane the pixel of source m that confirms it, or -1
  __shared__ int s_wave[kFuseWaves];
  const int tid = threadIdx.x;
  const int M = views.count;
  stage_view_poses(s_rel, poses, cams, views);
  if (tid <= M) {
    const int s = tid < M ? views.src[tid] : views.ref, slot = tid < M ? tid : kMaxSources;
#pragma unroll
    for (int c = 0; c < 12; ++c) s_pose[slot][c] = poses[12 * s + c];
  }
  __syncthreads();
  const long plane = (long)H * W;
  const long p = (long)blockIdx.x * kFuseThreads + tid;
  const bool live = p < plane;
  const long pc = live ? p : plane - 1;            // a lane past the frame works on the last pixel and stores nothing
  const int y = (int)(pc / W), x = (int)(pc - (long)y * W);
  const long vp = views.ref * plane + pc;
  const double z = (double)depth[vp];
  const bool seed = live && z > 0.0 && claimed[vp] == 0;
  const bool with_normals = normals != nullptr, with_rgb = frames != nullptr;
  int nv = 1;
  double X[3] = {0.0, 0.0, 0.0}, N[3] = {0.0, 0.0, 0.0}, C[3] = {0.0, 0.0, 0.0};
  double n_seed[3] = {0.0, 0.0, 0.0};
  bool seed_normal = false;
  if (seed) {
    const double* ray = rays + 2 * (views.ref_ray * plane + pc);
    const double P0 = ray[0] * z, P1 = ray[1] * z;
    {
      const double* T = s_pose[kMaxSources];
      const double q0 = P0 - T[3], q1 = P1 - T[7], q2 = z - T[11];
#pragma unroll
      for (int i = 0; i < 3; ++i) X[i] = T[i] * q0 + T[4 + i] * q1 + T[8 + i] * q2;
    }
    if (with_normals) {
#pragma unroll
      for (int i = 0; i < 3; ++i) n_seed[i] = (double)normals[3 * vp + i];
      seed_normal = n_seed[0] != 0.0 || n_seed[1] != 0.0 || n_seed[2] != 0.0;
      if (seed_normal) {
#pragma unroll
        for (int i = 0; i < 3; ++i) N[i] = n_seed[i];
      }
    }
    if (with_rgb) {
#pragma unroll
      for (int c = 0; c < 3; ++c) C[c] = (double)frames[(views.ref * 3L + c) * plane + pc];
    }
    for (int m = 0; m < M; ++m) {
      s_pix[m][tid] = -1;
      SourceHit hit;
      if (!source_confirms(s_rel, views, m, depth, rays, H, W, x, y, P0, P1, z, reproj_tol, rel_depth_tol, hit)) continue;
      const long ps = hit.ps, sp = views.src[m] * plane + ps;
      const double Q0 = hit.q0, Q1 = hit.q1, zs = hit.zs;
      double ns[3] = {0.0, 0.0, 0.0};
      bool src_normal = false;
      if (with_normals) {
#pragma unroll
        for (int i = 0; i < 3; ++i) ns[i] = (double)normals[3 * sp + i];
        src_normal = ns[0] != 0.0 || ns[1] != 0.0 || ns[2] != 0.0;
        if (seed_normal && src_normal && !(ns[0] * n_seed[0] + ns[1] * n_seed[1] + ns[2] * n_seed[2] >= min_normal_cos)) continue;
      }
      const double* T = s_pose[m];
      const double q0 = Q0 - T[3], q1 = Q1 - T[7], q2 = zs - T[11];
#pragma unroll
      for (int i = 0; i < 3; ++i) X[i] = X[i] + (T[i] * q0 + T[4 + i] * q1 + T[8 + i] * q2);
      if (src_normal) {
#pragma unroll
        for (int i = 0; i < 3; ++i) N[i] = N[i] + ns[i];
      }
      if (with_rgb) {
#pragma unroll
        for (int c = 0; c < 3; ++c) C[c] = C[c] + (double)frames[(views.src[m] * 3L + c) * plane + ps];
      }
      s_pix[m][tid] = (int)ps;
      ++nv;
    }
  }
  const bool emit = seed && nv >= min_views;
  if (emit) {
    for (int m = 0; m < M; ++m) {
      const int ps = s_pix[m][tid];
      if (ps >= 0) claimed[views.src[m] * plane + ps] = 1;
    }
    const double cnt = (double)nv;
#pragma unroll
    for (int i = 0; i < 3; ++i) stage_xyz[3 * p + i] = X[i] / cnt;
    if (with_normals) {
      const double l = sqrt(N[0] * N[0] + N[1] * N[1] + N[2] * N[2]);
#pragma unroll
      for (int i = 0; i < 3; ++i) stage_normal[3 * p + i] = l > 0.0 ? (float)(N[i] / l) : 0.0f;
    }
    if (with_rgb) {
#pragma unroll
      for (int c = 0; c < 3; ++c) stage_rgb[3 * p + c] = (float)(C[c] / cnt);
    }
  }
  if (live) stage_views[p] = emit ? nv : 0;
  int total;
  block_scan_flag<kFuseWaves>(emit, s_wave, &total);
  if (tid == 0) block_counts[blockIdx.x] = total;
}

// The staged points of a view to their rows: the workgroup's first row is count_in plus the counts of the workgroups
// before it (an integer sum, so its order is free), a lane's row the number of points before it in the workgroup.
__global__ __launch_bounds__(kFuseThreads) void fuse_compact_kernel(
    const int32_t* __restrict__ stage_views, const double* __restrict__ stage_xyz, const float* __restrict__ stage_normal,
    const float* __restrict__ stage_rgb, const int32_t* __restrict__ block_counts, long plane, int view,
    const int64_t* __restrict__ count_in, int64_t* __restrict__ count_out, long capacity, double* __restrict__ out_xyz,
    float* __restrict__ out_normal, float* __restrict__ out_rgb, int32_t* __restrict__ out_num_views,
    int32_t* __restrict__ out_view, int32_t* __restrict__ out_pixel) {
  __shared__ int s_wave[kFuseWaves];
  __shared__ int s_before[kFuseWaves];
  const int tid = threadIdx.x;
  int part = 0;
  for (int b = tid; b < (int)blockIdx.x; b += kFuseThreads) part += block_counts[b];
  part = wave_sum_i(part);
  if (lane_id() == 0) s_before[tid / kWave] = part;
  const long p = (long)blockIdx.x * kFuseThreads + tid;
  const int nv = p < plane ? stage_views[p] : 0;
  int total;
  const int pos = block_scan_flag<kFuseWaves>(nv > 0, s_wave, &total);   // (its barriers also publish s_before)
  long before = 0;
#pragma unroll
  for (int k = 0; k < kFuseWaves; ++k) before += s_before[k];
  const long first = (long)count_in[0] + before;
  const long row = first + pos;
  if (nv > 0 && row < capacity) {
#pragma unroll
    for (int i = 0; i < 3; ++i) out_xyz[3 * row + i] = stage_xyz[3 * p + i];
    if (stage_normal != nullptr) {
#pragma unroll
      for (int i = 0; i < 3; ++i) out_normal[3 * row + i] = stage_normal[3 * p + i];
    }
    if (stage_rgb != nullptr) {
#pragma unroll
      for (int i = 0; i < 3; ++i) out_rgb[3 * row + i] = stage_rgb[3 * p + i];
    }
    out_num_views[row] = nv;
    out_view[row] = view;
    out_pixel[row] = (int32_t)p;
  }
  if (blockIdx.x == gridDim.x - 1 && tid == 0) count_out[0] = (int64_t)(first + total);
}

}  // namespace vgg

using namespace vgg;

extern "C" {

const char* vggf_build_arch(void) { return "gfx950"; }

int vggf_depth_normals(const float* depth, const double* poses, const double* rays, const int32_t* ray_index, int num_rays,
                       int num_frames, int height, int width, double max_rel_jump, float* out_normals, void* stream) {
  if (height < 0 || width < 0 || !ray_index_ok(ray_index, num_frames, num_rays) || !(max_rel_jump >= 0.0))
    return VGG_ERR_INVALID_ARGUMENT;
  if (height == 0 || width == 0) return VGG_OK;
  if (!depth || !poses || !rays || !out_normals) return VGG_ERR_INVALID_ARGUMENT;
  if ((long)height * width > (long)INT32_MAX || div_up(height, kTile) > 65535) return VGG_ERR_UNSUPPORTED;
  for (int first = 0; first < num_frames; first += kNormalViews) {
    NormalViews views;
    memset(&views, 0, sizeof(views));
    views.first = first;
    const int count = num_frames - first < kNormalViews ? num_frames - first : kNormalViews;
    for (int i = 0; i < count; ++i) views.ray[i] = ray_index[first + i];
    const dim3 grid(div_up(width, kTile), div_up(height, kTile), count);
    fuse_normals_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(depth, poses, rays, height, width, views, max_rel_jump,
                                                               out_normals);
    VGG_LAUNCH_CHECK();
  }
  return VGG_OK;
}

int vggf_fuse_view(const float* depth, const float* normals, const float* frames, const double* poses, const double* cams,
                   const double* rays, const int32_t* ray_index, int num_rays, int num_frames, int height, int width,
                   int view, const int32_t* sources, int num_sources, double rel_depth_tol, double reproj_tol,
                   double min_normal_cos, int min_views, uint8_t* claimed, int32_t* stage_views, double* stage_xyz,
                   float* stage_normal, float* stage_rgb, int32_t* block_counts, const int64_t* count_in, int64_t* count_out,
                   long capacity, double* out_xyz, float* out_normal, float* out_rgb, int32_t* out_num_views,
                   int32_t* out_view, int32_t* out_pixel, void* stream) {
  DenseViews views;
  if (height < 0 || width < 0 || !ray_index || !make_views(num_frames, view, sources, num_sources, 0, ray_index, num_rays, &views))
    return VGG_ERR_INVALID_ARGUMENT;
  if (min_views < 1 || min_views > num_sources + 1 || !(rel_depth_tol >= 0.0) || !(reproj_tol >= 0.0) ||
      min_normal_cos != min_normal_cos || capacity < 0)
    return VGG_ERR_INVALID_ARGUMENT;
  if (height == 0 || width == 0) return VGG_OK;
  if (!depth || !poses || !cams || !rays || !claimed || !stage_views || !stage_xyz || !block_counts || !count_in || !count_out ||
      count_in == count_out || !out_xyz || !out_num_views || !out_view || !out_pixel)
    return VGG_ERR_INVALID_ARGUMENT;
  if ((normals && (!stage_normal || !out_normal)) || (frames && (!stage_rgb || !out_rgb))) return VGG_ERR_INVALID_ARGUMENT;
  const long plane = (long)height * width;
  if (plane > (long)INT32_MAX) return VGG_ERR_UNSUPPORTED;
  const int blocks = div_up(plane, kFuseThreads);
  hipStream_t st = (hipStream_t)stream;
  fuse_view_kernel<<<blocks, kFuseThreads, 0, st>>>(depth, normals, frames, poses, cams, rays, height, width, views,
                                                    rel_depth_tol, reproj_tol, min_normal_cos, min_views, claimed, stage_views,
                                                    stage_xyz, normals ? stage_normal : nullptr, frames ? stage_rgb : nullptr,
                                                    block_counts);
  VGG_LAUNCH_CHECK();
  fuse_compact_kernel<<<blocks, kFuseThreads, 0, st>>>(stage_views, stage_xyz, normals ? stage_normal : nullptr,
                                                       frames ? stage_rgb : nullptr, block_counts, plane, view, count_in,
                                                       count_out, capacity, out_xyz, out_normal, out_rgb, out_num_views,
                                                       out_view, out_pixel);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

}  // extern "C"
