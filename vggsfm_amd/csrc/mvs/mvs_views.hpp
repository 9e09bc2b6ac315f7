// The views of one call of the dense stage and the forward-backward confirmation of a pixel by a source: one copy, included
// by mvs.hip, ../patchmatch/patchmatch.hip and ../fuse/fuse.hip (all parity files, built with -ffp-contract=off).
#pragma once
#include <stdint.h>
#include <string.h>

#include "mvs_geometry.hpp"

namespace vgg {

constexpr int kMaxSources = 8;   // VGGM_ / VGGR_ / VGGF_MAX_SOURCES of the three headers

// by-value kernel argument: the reference (or the view to fuse), up to 8 sources and everyone's ray map (validated on the host)
struct DenseViews {
  int32_t src[kMaxSources];
  int32_t src_ray[kMaxSources];
  int32_t ref, ref_ray, count;
};

// every frame names a ray map that exists; false without a table too
inline bool ray_index_ok(const int32_t* ray_index, int num_frames, int num_rays) {
  if (!ray_index || num_rays < 1 || num_frames < 1) return false;
  for (int s = 0; s < num_frames; ++s)
    if (ray_index[s] < 0 || ray_index[s] >= num_rays) return false;
  return true;
}

// The views of a call from its host arrays; false: refused.  min_sources is 1, or 0 where a view may stand alone (fusion);
// ray_index is null for an entry whose rays belong to the reference alone (the sweep, PatchMatch): the ray maps then stay 0.
inline bool make_views(int num_frames, int ref, const int32_t* sources, int num_sources, int min_sources,
                       const int32_t* ray_index, int num_rays, DenseViews* v) {
  if (num_frames < 1 || ref < 0 || ref >= num_frames || num_sources < min_sources || num_sources > kMaxSources ||
      (num_sources > 0 && !sources))
    return false;
  memset(v, 0, sizeof(*v));
  v->ref = ref;
  v->count = num_sources;
  for (int m = 0; m < num_sources; ++m) {
    if (sources[m] < 0 || sources[m] >= num_frames || sources[m] == ref) return false;
    v->src[m] = sources[m];
  }
  if (ray_index) {
    if (!ray_index_ok(ray_index, num_frames, num_rays)) return false;
    v->ref_ray = ray_index[ref];
    for (int m = 0; m < num_sources; ++m) v->src_ray[m] = ray_index[sources[m]];
  }
  return true;
}

// in LDS: both relative poses of every source and the cameras
struct ViewPoses {
  double fwd[kMaxSources][12];      // source from ref
  double bwd[kMaxSources][12];      // ref from source
  double cam[kMaxSources + 1][4];   // the sources', then ref's
};

// lanes m < count derive both relative poses of source m and copy its camera, lanes < 4 the reference's; the caller's
// barrier follows
__device__ __forceinline__ void stage_view_poses(ViewPoses& s, const double* __restrict__ poses,
                                                 const double* __restrict__ cams, const DenseViews& views) {
  const int tid = threadIdx.x;
  if (tid < views.count) {
    const int src = views.src[tid];
    relative_pose(poses + 12 * views.ref, poses + 12 * src, s.fwd[tid]);
    relative_pose(poses + 12 * src, poses + 12 * views.ref, s.bwd[tid]);
#pragma unroll
    for (int c = 0; c < 4; ++c) s.cam[tid][c] = cams[4 * src + c];
  }
  if (tid < 4) s.cam[kMaxSources][tid] = cams[4 * views.ref + tid];
}

// the source pixel that confirms a reference pixel, and its camera-frame point
struct SourceHit {
  long ps;
  double q0, q1, zs;
};

// Does source m confirm the reference's pixel (x, y) with depth z > 0 and camera-frame point (p0, p1, z)?  Forwards into
// the source, to the nearest pixel, whose own depth must be positive; that pixel's point comes back into the reference
// within reproj_tol pixels of (x, y) and rel_depth_tol of z.  `hit` is set on true.
__device__ __forceinline__ bool source_confirms(const ViewPoses& s, const DenseViews& views, int m,
                                                const float* __restrict__ depth, const double* __restrict__ rays, int H, int W,
                                                int x, int y, double p0, double p1, double z, double reproj_tol,
                                                double rel_depth_tol, SourceHit& hit) {
  const long plane = (long)H * W;
  double xs, ys, zc;
  if (!transfer_project(s.fwd[m], s.cam[m], p0, p1, z, xs, ys, zc)) return false;
  const double xi = floor(xs + 0.5), yi = floor(ys + 0.5);
  if (!inside_image(xi, yi, H, W)) return false;
  const long ps = (long)yi * W + (long)xi;
  const double zs = (double)depth[views.src[m] * plane + ps];
  if (!(zs > 0.0)) return false;
  const double* rs = rays + 2 * (views.src_ray[m] * plane + ps);
  const double q0 = rs[0] * zs, q1 = rs[1] * zs;
  hit = {ps, q0, q1, zs};
  double xb, yb, zb;
  if (!transfer_project(s.bwd[m], s.cam[kMaxSources], q0, q1, zs, xb, yb, zb)) return false;
  const double ex = xb - (double)x, ey = yb - (double)y;
  return sqrt(ex * ex + ey * ey) <= reproj_tol && fabs(zb - z) / z <= rel_depth_tol;
}

}  // namespace vgg
