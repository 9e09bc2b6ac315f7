// A z-buffer rasteriser of triangle meshes for gfx950: the entries of vggsfm_amd_raster.h.
// A parity file: built with -ffp-contract=off, every expression in the header's order (tests/render_cases.py restates it in
// NumPy, testing every pixel against every face).
#include <math.h>

#include "../common.hpp"
#include "../mvs/mvs_views.hpp"
#include "vggsfm_amd_raster.h"

namespace vgg {

constexpr int kMaxViews = VGGZ_MAX_VIEWS;
// (VGGZ_SOLO_OVERRIDE and VGGZ_NO_EARLY_OUT are set by scripts/time_render.py in builds of its own, never in the library)
#ifdef VGGZ_SOLO_OVERRIDE
constexpr int kSoloPixels = VGGZ_SOLO_OVERRIDE;
#else
constexpr int kSoloPixels = VGGZ_SOLO_PIXELS;
#endif
constexpr unsigned long long kEmptyKey = ~0ull;

// by-value kernel argument, validated on the host: the views of a launch and the ray map of each
struct RasterViews {
  int32_t first;
  int32_t ray[kMaxViews];
};

// A face in one view: the normalised image points and inverse depths of its vertices; bit e of flags: edge e (0: 1 -> 2,
// 1: 2 -> 0, 2: 0 -> 1) runs from the higher vertex row to the lower one; bit 3: sigma = -1.  (Scalars, no arrays: a select
// between two elements of a private array is a pointer the compiler cannot keep in registers.)
struct FaceSetup {
  double a0, a1, a2, b0, b1, b2, iz0, iz1, iz2;
  int flags;
};

// An edge as the pixel loop wants it: its lower-row end (ap, bp), the step to its higher-row end (da, db) and the sign
// sg = +1 or -1 that turns e_pq into w.
struct Edge {
  double ap, bp, da, db, sg;
};
struct FaceEdges {
  Edge e0, e1, e2;
  double iz0, iz1, iz2;
};

// the vertex rows of a face; false: a row outside [0, V) or two equal rows (no vertex is loaded)
__device__ __forceinline__ bool face_rows(const int32_t* __restrict__ face, int V, int& i0, int& i1, int& i2) {
  i0 = face[0];
  i1 = face[1];
  i2 = face[2];
  if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) return false;
  return i0 != i1 && i1 != i2 && i0 != i2;
}

// iz, a, b of vertex `row`; z: Xc[2]
__device__ __forceinline__ void vertex_point(const double* __restrict__ vertices, int row, const double* pose, double& a, double& b,
                                             double& iz, double& z) {
  const double* P = vertices + 3 * (long)row;
  double X0, X1;
  transfer(pose, P[0], P[1], P[2], X0, X1, z);
  iz = 1.0 / z;
  a = X0 * iz;
  b = X1 * iz;
}

// n_j, iz_j and the edge directions of a face with valid rows; `front`: Xc_j[2] > near for j = 0, 1, 2; sigma is not
// decided here
__device__ __forceinline__ void face_points(const double* __restrict__ vertices, int i0, int i1, int i2, const double* pose,
                                            double near, FaceSetup& f, bool& front) {
  double z0, z1, z2;
  vertex_point(vertices, i0, pose, f.a0, f.b0, f.iz0, z0);
  vertex_point(vertices, i1, pose, f.a1, f.b1, f.iz1, z1);
  vertex_point(vertices, i2, pose, f.a2, f.b2, f.iz2, z2);
  front = z0 > near && z1 > near && z2 > near;
  f.flags = (i1 > i2 ? 1 : 0) | (i2 > i0 ? 2 : 0) | (i0 > i1 ? 4 : 0);
}

// the edge from (au, bu) to (av, bv); rev: u has the higher row; neg: sigma = -1
__device__ __forceinline__ Edge make_edge(double au, double bu, double av, double bv, bool rev, bool neg) {
  Edge e;
  e.ap = rev ? av : au;
  e.bp = rev ? bv : bu;
  e.da = (rev ? au : av) - e.ap;
  e.db = (rev ? bu : bv) - e.bp;
  e.sg = rev != neg ? -1.0 : 1.0;
  return e;
}

__device__ __forceinline__ FaceEdges face_edges(const FaceSetup& f) {
  FaceEdges E;
  const bool neg = (f.flags & 8) != 0;
  E.e0 = make_edge(f.a1, f.b1, f.a2, f.b2, (f.flags & 1) != 0, neg);
  E.e1 = make_edge(f.a2, f.b2, f.a0, f.b0, (f.flags & 2) != 0, neg);
  E.e2 = make_edge(f.a0, f.b0, f.a1, f.b1, (f.flags & 4) != 0, neg);
  E.iz0 = f.iz0;
  E.iz1 = f.iz1;
  E.iz2 = f.iz2;
  return E;
}

// w_e = sg_e e_pq(a, b)
__device__ __forceinline__ double edge_weight(const Edge& e, double a, double b) {
  return e.sg * (e.da * (b - e.bp) - e.db * (a - e.ap));
}

// sigma from A = E(0 -> 1) at n_2; false unless A > 0 or A < 0
__device__ __forceinline__ bool face_sigma(FaceSetup& f) {
  const double A = edge_weight(make_edge(f.a0, f.b0, f.a1, f.b1, (f.flags & 4) != 0, false), f.a2, f.b2);
  if (!(A > 0.0 || A < 0.0)) return false;
  if (A < 0.0) f.flags |= 8;
  return true;
}

// lambda_j and q at the ray (a, b); true: covered (w0, w1, w2 >= 0 and sum > 0)
__device__ __forceinline__ bool face_weights(const FaceEdges& E, double a, double b, double& l0, double& l1, double& l2,
                                             double& q) {
  const double w0 = edge_weight(E.e0, a, b), w1 = edge_weight(E.e1, a, b), w2 = edge_weight(E.e2, a, b);
  const double sum = (w0 + w1) + w2;
  l0 = w0 / sum;
  l1 = w1 / sum;
  l2 = w2 / sum;
  q = (l0 * E.iz0 + l1 * E.iz1) + l2 * E.iz2;
  return w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0 && sum > 0.0;
}

// the header's candidate box, clamped to the frame; false: it misses the frame or is not finite
__device__ __forceinline__ bool face_box(const FaceSetup& f, const double* cam, int H, int W, int& x0, int& y0, int& bw,
                                         int& count) {
  double px0, py0, px1, py1, px2, py2;
  project_normalised(cam, f.a0, f.b0, px0, py0);
  project_normalised(cam, f.a1, f.b1, px1, py1);
  project_normalised(cam, f.a2, f.b2, px2, py2);
  const double xmin = fmin(fmin(px0, px1), px2), xmax = fmax(fmax(px0, px1), px2);
  const double ymin = fmin(fmin(py0, py1), py2), ymax = fmax(fmax(py0, py1), py2);
  const bool finite = (px0 + px1 + px2) - (px0 + px1 + px2) == 0.0 && (py0 + py1 + py2) - (py0 + py1 + py2) == 0.0;
  const double r2 = fmax(fmax(f.a0 * f.a0 + f.b0 * f.b0, f.a1 * f.a1 + f.b1 * f.b1), f.a2 * f.a2 + f.b2 * f.b2);
  const double d0a = f.a1 - f.a0, d0b = f.b1 - f.b0, d1a = f.a2 - f.a1, d1b = f.b2 - f.b1, d2a = f.a0 - f.a2, d2b = f.b0 - f.b2;
  const double L2 = fmax(fmax(d0a * d0a + d0b * d0b, d1a * d1a + d1b * d1b), d2a * d2a + d2b * d2b);
  const double m = 1.0 + 0.75 * cam[0] * fabs(cam[3]) * sqrt(r2) * L2;
  const double bx0 = floor(xmin - m), bx1 = ceil(xmax + m), by0 = floor(ymin - m), by1 = ceil(ymax + m);
  if (!(finite && m >= 1.0 && bx1 >= 0.0 && bx0 <= (double)(W - 1) && by1 >= 0.0 && by0 <= (double)(H - 1))) return false;
  x0 = (int)fmax(bx0, 0.0);
  y0 = (int)fmax(by0, 0.0);
  const int x1 = (int)fmin(bx1, (double)(W - 1)), y1 = (int)fmin(by1, (double)(H - 1));
  bw = x1 - x0 + 1;
  count = bw * (y1 - y0 + 1);                          // <= H W <= INT32_MAX
  return true;
}

// pixel (x, y) of the frame against one face: THE RULE from the ray on
__device__ __forceinline__ void draw_pixel(const FaceEdges& E, const double* __restrict__ rm, unsigned long long* km, int W,
                                           int x, int y, unsigned g) {
  const long p = (long)y * W + x;
  double l0, l1, l2, q;
  if (!face_weights(E, rm[2 * p], rm[2 * p + 1], l0, l1, l2, q)) return;
  const float zf = (float)(1.0 / q);
  if (!(zf > 0.0f && zf < INFINITY)) return;
  const unsigned long long key = (unsigned long long)__float_as_uint(zf) << 32 | g;
#ifndef VGGZ_NO_EARLY_OUT
  // keys only fall: a stale read is only ever too large, so it costs a superfluous atomic and never loses one
  if (key >= __atomic_load_n(km + p, __ATOMIC_RELAXED)) return;
#endif
  atomicMin(km + p, key);
}

// ------------------------------------------------------------------------------------------------------------ raster
// One lane per (face, view), the view on the grid's y axis: poses and cameras sit at wave-uniform addresses.  Faces with a
// box of at most kSoloPixels pixels are walked by their lane; the wavefront then takes the larger ones in lane order, the
// owner's set-up broadcast and the 64 lanes striding over the box.  No LDS, no list, no second launch.
__global__ __launch_bounds__(256) void raster_kernel(const double* __restrict__ vertices, int V, const int32_t* __restrict__ faces,
                                                     int F, int face_base, const double* __restrict__ poses,
                                                     const double* __restrict__ cams, const double* __restrict__ rays,
                                                     RasterViews views, int H, int W, double near, unsigned long long* keys) {
  const long s = (long)views.first + blockIdx.y;
  const long plane = (long)H * W;
  const double* pose = poses + 12 * s;
  const double* cam = cams + 4 * s;
  const double* rm = rays + 2 * ((long)views.ray[blockIdx.y] * plane);
  unsigned long long* km = keys + s * plane;
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  FaceSetup f;
  memset(&f, 0, sizeof(f));
  int x0 = 0, y0 = 0, bw = 1, count = 0;
  bool ok = r < F;
  if (ok) {
    int i0, i1, i2;
    ok = face_rows(faces + 3 * r, V, i0, i1, i2);
    if (ok) {
      face_points(vertices, i0, i1, i2, pose, near, f, ok);
      ok = ok && face_sigma(f) && face_box(f, cam, H, W, x0, y0, bw, count);
    }
  }
  if (!ok) count = 0;
  const unsigned g = (unsigned)face_base + (unsigned)r;
  if (count > 0 && count <= kSoloPixels) {
    const FaceEdges E = face_edges(f);
    int x = x0, y = y0;
    for (int i = 0; i < count; ++i) {
      draw_pixel(E, rm, km, W, x, y, g);
      if (++x == x0 + bw) {
        x = x0;
        ++y;
      }
    }
  }
  // every lane of the wavefront is here: the loop below is wave-uniform
  unsigned long long large = __ballot(count > kSoloPixels);
  const int lane = lane_id();
  while (large != 0ull) {
    const int src = __ffsll((long long)large) - 1;
    large &= large - 1ull;
    FaceSetup fs;
    fs.a0 = wave_bcast(f.a0, src);
    fs.a1 = wave_bcast(f.a1, src);
    fs.a2 = wave_bcast(f.a2, src);
    fs.b0 = wave_bcast(f.b0, src);
    fs.b1 = wave_bcast(f.b1, src);
    fs.b2 = wave_bcast(f.b2, src);
    fs.iz0 = wave_bcast(f.iz0, src);
    fs.iz1 = wave_bcast(f.iz1, src);
    fs.iz2 = wave_bcast(f.iz2, src);
    fs.flags = __builtin_amdgcn_readlane(f.flags, src);
    const int sx0 = __builtin_amdgcn_readlane(x0, src), sy0 = __builtin_amdgcn_readlane(y0, src);
    const int sbw = __builtin_amdgcn_readlane(bw, src), scount = __builtin_amdgcn_readlane(count, src);
    const unsigned sg = (unsigned)__builtin_amdgcn_readlane((int)g, src);
    const FaceEdges E = face_edges(fs);
    for (int i = lane; i < scount; i += kWave) {
      const int row = i / sbw;
      draw_pixel(E, rm, km, W, sx0 + (i - row * sbw), sy0 + row, sg);
    }
  }
}

// ----------------------------------------------------------------------------------------------------------- resolve
// One lane per pixel and view: the face and the depth from the key, the weights recomputed by the raster's own code.
__global__ __launch_bounds__(256) void resolve_kernel(const unsigned long long* __restrict__ keys, const double* __restrict__ vertices,
                                                      int V, const int32_t* __restrict__ faces, int F,
                                                      const float* __restrict__ vertex_normals, const float* __restrict__ vertex_rgb,
                                                      const double* __restrict__ poses, const double* __restrict__ rays,
                                                      RasterViews views, int H, int W, float* __restrict__ out_depth,
                                                      int32_t* __restrict__ out_face, double* __restrict__ out_weights,
                                                      float* __restrict__ out_normal, float* __restrict__ out_rgb) {
  const long plane = (long)H * W;
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= plane) return;
  const long s = (long)views.first + blockIdx.y;
  const long o = s * plane + p;
  const unsigned long long key = keys[o];
  const unsigned g = (unsigned)key;
  int i0 = 0, i1 = 0, i2 = 0;
  const bool hit = key != kEmptyKey && g < (unsigned)F && face_rows(faces + 3 * (long)g, V, i0, i1, i2);
  float depth = 0.0f;
  int32_t face = -1;
  double o0 = 0.0, o1 = 0.0, o2 = 0.0;
  if (hit) {
    FaceSetup f;
    bool front;                                        // (not used: the raster drew the face, so it passed the test)
    face_points(vertices, i0, i1, i2, poses + 12 * s, 0.0, f, front);
    face_sigma(f);
    const FaceEdges E = face_edges(f);
    const double* ray = rays + 2 * ((long)views.ray[blockIdx.y] * plane + p);
    double l0, l1, l2, q;
    face_weights(E, ray[0], ray[1], l0, l1, l2, q);
    o0 = (l0 * E.iz0) / q;
    o1 = (l1 * E.iz1) / q;
    o2 = (l2 * E.iz2) / q;
    depth = __uint_as_float((unsigned)(key >> 32));
    face = (int32_t)g;
  }
  out_depth[o] = depth;
  out_face[o] = face;
  if (out_weights != nullptr) {
    out_weights[3 * o] = o0;
    out_weights[3 * o + 1] = o1;
    out_weights[3 * o + 2] = o2;
  }
  if (vertex_normals != nullptr) {
    double G[3] = {0.0, 0.0, 0.0};
    if (hit) {
      const float *N0 = vertex_normals + 3 * (long)i0, *N1 = vertex_normals + 3 * (long)i1, *N2 = vertex_normals + 3 * (long)i2;
#pragma unroll
      for (int c = 0; c < 3; ++c) G[c] = (o0 * (double)N0[c] + o1 * (double)N1[c]) + o2 * (double)N2[c];
    }
    const double len = sqrt((G[0] * G[0] + G[1] * G[1]) + G[2] * G[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) out_normal[3 * o + c] = len > 0.0 ? (float)(G[c] / len) : 0.0f;
  }
  if (vertex_rgb != nullptr) {
    double G[3] = {0.0, 0.0, 0.0};
    if (hit) {
      const float *C0 = vertex_rgb + 3 * (long)i0, *C1 = vertex_rgb + 3 * (long)i1, *C2 = vertex_rgb + 3 * (long)i2;
#pragma unroll
      for (int c = 0; c < 3; ++c) G[c] = (o0 * (double)C0[c] + o1 * (double)C1[c]) + o2 * (double)C2[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out_rgb[3 * o + c] = (float)G[c];
  }
}

// -------------------------------------------------------------------------------------------------------- visibility
// One lane per point, the view on the grid's y axis.
__global__ __launch_bounds__(256) void visibility_kernel(const double* __restrict__ points, int P, const float* __restrict__ depth,
                                                         const double* __restrict__ poses, const double* __restrict__ cams, int first,
                                                         int H, int W, double rel_tol, uint8_t* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  const long s = (long)first + blockIdx.y;
  double x, y, zc;
  bool visible = transfer_project(poses + 12 * s, cams + 4 * s, points[3 * i], points[3 * i + 1], points[3 * i + 2], x, y, zc);
  const double xi = floor(x + 0.5), yi = floor(y + 0.5);
  visible = visible && inside_image(xi, yi, H, W);
  if (visible) {
    const double zr = (double)depth[s * ((long)H * W) + (long)yi * W + (long)xi];
    visible = zr > 0.0 && zc <= zr * (1.0 + rel_tol);
  }
  out[s * (long)P + i] = visible ? 1 : 0;
}

static RasterViews launch_views(const int32_t* ray_index, int first, int count) {
  RasterViews v;
  memset(&v, 0, sizeof(v));
  v.first = first;
  for (int i = 0; i < count; ++i) v.ray[i] = ray_index[first + i];
  return v;
}

}  // namespace vgg

using namespace vgg;

extern "C" {

const char* vggz_build_arch(void) { return "gfx950"; }

int vggz_raster(const double* vertices, int num_vertices, const int32_t* faces, int num_faces, int face_base,
                const double* poses, const double* cams, const double* rays, const int32_t* ray_index, int num_rays,
                int num_frames, int height, int width, double near, uint64_t* keys, void* stream) {
  if (!(near > 0.0) || num_vertices < 0 || num_faces < 0 || height < 0 || width < 0 || face_base < 0 ||
      (long)face_base + num_faces > (long)INT32_MAX || !ray_index_ok(ray_index, num_frames, num_rays))
    return VGG_ERR_INVALID_ARGUMENT;
  if (num_faces == 0 || num_vertices == 0 || height == 0 || width == 0) return VGG_OK;
  if (!vertices || !faces || !poses || !cams || !rays || !keys) return VGG_ERR_INVALID_ARGUMENT;
  if ((long)height * width > (long)INT32_MAX) return VGG_ERR_UNSUPPORTED;
  for (int first = 0; first < num_frames; first += kMaxViews) {
    const int count = num_frames - first < kMaxViews ? num_frames - first : kMaxViews;
    const dim3 grid(div_up(num_faces, 256), count);
    raster_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(vertices, num_vertices, faces, num_faces, face_base, poses, cams, rays,
                                                         launch_views(ray_index, first, count), height, width, near,
                                                         (unsigned long long*)keys);
    VGG_LAUNCH_CHECK();
  }
  return VGG_OK;
}

int vggz_resolve(const uint64_t* keys, const double* vertices, int num_vertices, const int32_t* faces, int num_faces_total,
                 const float* vertex_normals, const float* vertex_rgb, const double* poses, const double* rays,
                 const int32_t* ray_index, int num_rays, int num_frames, int height, int width, float* out_depth,
                 int32_t* out_face, double* out_weights, float* out_normal, float* out_rgb, void* stream) {
  if (num_vertices < 0 || num_faces_total < 0 || height < 0 || width < 0 || !ray_index_ok(ray_index, num_frames, num_rays) ||
      (vertex_normals && !out_normal) || (vertex_rgb && !out_rgb))
    return VGG_ERR_INVALID_ARGUMENT;
  if (height == 0 || width == 0) return VGG_OK;
  if (!keys || !poses || !rays || !out_depth || !out_face || (num_vertices > 0 && !vertices) || (num_faces_total > 0 && !faces))
    return VGG_ERR_INVALID_ARGUMENT;
  if ((long)height * width > (long)INT32_MAX) return VGG_ERR_UNSUPPORTED;
  for (int first = 0; first < num_frames; first += kMaxViews) {
    const int count = num_frames - first < kMaxViews ? num_frames - first : kMaxViews;
    const dim3 grid(div_up((long)height * width, 256), count);
    resolve_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((const unsigned long long*)keys, vertices, num_vertices, faces,
                                                          num_faces_total, vertex_normals, vertex_rgb, poses, rays,
                                                          launch_views(ray_index, first, count), height, width, out_depth,
                                                          out_face, out_weights, out_normal, out_rgb);
    VGG_LAUNCH_CHECK();
  }
  return VGG_OK;
}

int vggz_point_visibility(const double* points, int num_points, const float* depth, const double* poses, const double* cams,
                          int num_frames, int height, int width, double rel_tol, uint8_t* out, void* stream) {
  if (!(rel_tol >= 0.0) || num_frames < 1 || num_points < 0 || height < 0 || width < 0) return VGG_ERR_INVALID_ARGUMENT;
  if (num_points == 0) return VGG_OK;
  if (!points || !poses || !cams || !out || ((long)height * width > 0 && !depth)) return VGG_ERR_INVALID_ARGUMENT;
  if ((long)height * width > (long)INT32_MAX) return VGG_ERR_UNSUPPORTED;
  for (int first = 0; first < num_frames; first += kMaxViews) {
    const int count = num_frames - first < kMaxViews ? num_frames - first : kMaxViews;
    const dim3 grid(div_up(num_points, 256), count);
    visibility_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(points, num_points, depth, poses, cams, first, height, width, rel_tol,
                                                             out);
    VGG_LAUNCH_CHECK();
  }
  return VGG_OK;
}

}  // extern "C"
