// A surface from depth maps for gfx950: TSDF integration and marching tetrahedra, the entries of vggsfm_amd_tsdf.h.
// A parity file: built with -ffp-contract=off, every sum in a stated order (tests/meshing_cases.py restates it in NumPy).
#include <math.h>

#include "../common.hpp"
#include "../scan.hpp"
#include "../mvs/mvs_geometry.hpp"
#include "vggsfm_amd_tsdf.h"

namespace vgg {

constexpr int kGroup = VGGV_GROUP, kGroupWaves = kGroup / kWave;   // one workgroup of count / emit = one group of nodes
constexpr int kMaxViews = VGGV_MAX_VIEWS;
constexpr int kScanThreads = 1024, kScanWaves = kScanThreads / kWave;
constexpr long kMaxNodes = (long)INT32_MAX / 7;

struct Grid {
  double o[3], h;
  int nx, ny, nz;
  long N;
};

// The 16 cases per orientation, written out: [sigma = +1, sigma = -1][case][number of triangles, then 3 edges per triangle],
// edges of the tetrahedron numbered (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); tests/meshing_cases.py derives the same table from
// the header's rule and tests/test_meshing_host.py compares the two through vggv_case_table.
#define VGGV_CASES                                                                                                       \
  {{{0, -1, -1, -1, -1, -1, -1}, {1, 0, 1, 2, -1, -1, -1}, {1, 0, 4, 3, -1, -1, -1}, {2, 1, 2, 4, 1, 4, 3},              \
    {1, 1, 3, 5, -1, -1, -1},    {2, 3, 5, 2, 3, 2, 0},    {2, 0, 4, 5, 0, 5, 1},    {1, 2, 4, 5, -1, -1, -1},           \
    {1, 2, 5, 4, -1, -1, -1},    {2, 0, 1, 5, 0, 5, 4},    {2, 2, 5, 3, 2, 3, 0},    {1, 1, 5, 3, -1, -1, -1},           \
    {2, 1, 3, 4, 1, 4, 2},       {1, 0, 3, 4, -1, -1, -1}, {1, 0, 2, 1, -1, -1, -1}, {0, -1, -1, -1, -1, -1, -1}},       \
   {{0, -1, -1, -1, -1, -1, -1}, {1, 0, 2, 1, -1, -1, -1}, {1, 0, 3, 4, -1, -1, -1}, {2, 3, 4, 2, 3, 2, 1},              \
    {1, 1, 5, 3, -1, -1, -1},    {2, 0, 2, 5, 0, 5, 3},    {2, 1, 5, 4, 1, 4, 0},    {1, 2, 5, 4, -1, -1, -1},           \
    {1, 2, 4, 5, -1, -1, -1},    {2, 4, 5, 1, 4, 1, 0},    {2, 0, 3, 5, 0, 5, 2},    {1, 1, 3, 5, -1, -1, -1},           \
    {2, 2, 4, 3, 2, 3, 1},       {1, 0, 4, 3, -1, -1, -1}, {1, 0, 1, 2, -1, -1, -1}, {0, -1, -1, -1, -1, -1, -1}}}
static const int8_t h_cases[2][16][7] = VGGV_CASES;
__constant__ int8_t d_cases[2][16][7] = VGGV_CASES;

// Small tables as nibbles of a constant (entry x = (word >> 4 x) & 7), so that a run-time index costs a shift and no
// indexed array.  A corner or a neighbour of a node is named by its code dx + 2 dy + 4 dz.
constexpr unsigned kEdgeCode = 0x7653421u;     // edge number 0 .. 6 -> code of its direction
constexpr unsigned kCodeEdge = 0x65423100u;    // code 1 .. 7 -> edge number
constexpr unsigned kTetC1 = 0x442211u;         // tetrahedron 0 .. 5 -> code of corner p1
constexpr unsigned kTetC2 = 0x656353u;         //                    -> code of corner p2 (p0 = 0, p3 = 7)
constexpr unsigned kTetOdd = 0x26u;            // bit t set: sigma = -1 (the permutations (0,2,1), (1,0,2), (2,1,0))
constexpr unsigned kEdgeLo = 0x211000u;        // tetrahedron edge 0 .. 5 -> its lower corner
constexpr unsigned kEdgeHi = 0x332321u;        //                         -> its higher corner

__device__ __forceinline__ int nib(unsigned word, int x) { return (int)((word >> (4 * x)) & 7u); }

__device__ __forceinline__ long code_offset(int code, int nx, int ny) {
  return (long)(code & 1) + (long)((code >> 1) & 1) * nx + (long)((code >> 2) & 1) * ((long)nx * ny);
}

// validity and value of node n (n inside the grid)
__device__ __forceinline__ bool node_value(const double* __restrict__ tsdf, const double* __restrict__ wsum, long n,
                                           double min_weight, double& s) {
  const double w = wsum[n];
  s = tsdf[n] / w;
  return w >= min_weight;
}

// ------------------------------------------------------------------------------------------------------- integration
// One lane per node; the views of the launch in order, their poses and cameras read at wave-uniform addresses.
__global__ __launch_bounds__(256) void tsdf_integrate_kernel(const float* __restrict__ depth, const float* __restrict__ weights,
                                                             const float* __restrict__ frames, const double* __restrict__ poses,
                                                             const double* __restrict__ cams, int first, int count, int H, int W,
                                                             Grid g, double trunc, double* __restrict__ tsdf_sum,
                                                             double* __restrict__ weight_sum, double* __restrict__ rgb_sum) {
  const long n = (long)blockIdx.x * 256 + threadIdx.x;
  if (n >= g.N) return;
  const long slab = (long)g.nx * g.ny;
  const int k = (int)(n / slab);
  const int j = (int)((n - k * slab) / g.nx), i = (int)(n - k * slab - (long)j * g.nx);
  const double X0 = g.o[0] + g.h * (double)i, X1 = g.o[1] + g.h * (double)j, X2 = g.o[2] + g.h * (double)k;
  const bool with_rgb = frames != nullptr && rgb_sum != nullptr;
  const long plane = (long)H * W;
  double ts = tsdf_sum[n], ws = weight_sum[n];
  double c0 = 0.0, c1 = 0.0, c2 = 0.0;
  if (with_rgb) {
    c0 = rgb_sum[3 * n];
    c1 = rgb_sum[3 * n + 1];
    c2 = rgb_sum[3 * n + 2];
  }
  for (int v = 0; v < count; ++v) {
    const long s = (long)first + v;
    double x, y, zc;
    if (!transfer_project(poses + 12 * s, cams + 4 * s, X0, X1, X2, x, y, zc)) continue;
    const double xi = floor(x + 0.5), yi = floor(y + 0.5);
    if (!inside_image(xi, yi, H, W)) continue;
    const long p = (long)yi * W + (long)xi;
    const double z = (double)depth[s * plane + p];
    if (!(z > 0.0)) continue;
    const double w = weights != nullptr ? (double)weights[s * plane + p] : 1.0;
    if (!(w > 0.0)) continue;
    const double sdf = z - zc;
    if (!(sdf >= -trunc)) continue;
    const double d = fmin(1.0, sdf / trunc);
    ts = ts + w * d;
    ws = ws + w;
    if (with_rgb) {
      const float* f = frames + (s * 3) * plane + p;
      c0 = c0 + w * (double)f[0];
      c1 = c1 + w * (double)f[plane];
      c2 = c2 + w * (double)f[2 * plane];
    }
  }
  tsdf_sum[n] = ts;
  weight_sum[n] = ws;
  if (with_rgb) {
    rgb_sum[3 * n] = c0;
    rgb_sum[3 * n + 1] = c1;
    rgb_sum[3 * n + 2] = c2;
  }
}

// ------------------------------------------------------------------------------------------------------- counting
// validity (bit c of vbits) and insideness (bit c of ibits) of the eight nodes n + code c that exist; a code whose node does
// not exist reads node n itself and counts as invalid
__device__ __forceinline__ void corner_bits(const double* __restrict__ tsdf, const double* __restrict__ wsum, long n, int i,
                                            int j, int k, int nx, int ny, int nz, double min_weight, unsigned& vbits,
                                            unsigned& ibits) {
  vbits = ibits = 0u;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const bool exists = i + (c & 1) < nx && j + ((c >> 1) & 1) < ny && k + ((c >> 2) & 1) < nz;
    double s;
    const bool valid = node_value(tsdf, wsum, exists ? n + code_offset(c, nx, ny) : n, min_weight, s) && exists;
    vbits |= (valid ? 1u : 0u) << c;
    ibits |= (valid && s < 0.0 ? 1u : 0u) << c;
  }
}

__device__ __forceinline__ unsigned edge_mask_of(unsigned vbits, unsigned ibits) {
  unsigned m = 0u;
#pragma unroll
  for (int e = 0; e < 7; ++e) {
    const int c = nib(kEdgeCode, e);
    const bool vertex = (vbits & 1u) && ((vbits >> c) & 1u) && ((ibits & 1u) != ((ibits >> c) & 1u));
    m |= (vertex ? 1u : 0u) << e;
  }
  return m;
}

// corner codes of tetrahedron t packed as nibbles p0 | p1 << 4 | p2 << 8 | p3 << 12; false: a corner is invalid
__device__ __forceinline__ bool tet_pattern(int t, unsigned vbits, unsigned ibits, unsigned& codes, int& pattern) {
  codes = (unsigned)nib(kTetC1, t) << 4 | (unsigned)nib(kTetC2, t) << 8 | 7u << 12;
  bool all = true;
  pattern = 0;
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const int c = nib(codes, x);
    all = all && ((vbits >> c) & 1u);
    pattern |= (int)((ibits >> c) & 1u) << x;
  }
  return all;
}

// One lane per node: its edge mask, and the prefix sums of vertices and faces inside its group.
__global__ __launch_bounds__(kGroup) void mesh_count_kernel(const double* __restrict__ tsdf, const double* __restrict__ wsum,
                                                            int nx, int ny, int nz, long N, double min_weight,
                                                            uint8_t* __restrict__ edge_mask, int32_t* __restrict__ vertex_offset,
                                                            int32_t* __restrict__ face_offset, int32_t* __restrict__ group_counts) {
  __shared__ int s_wv[kGroupWaves], s_wf[kGroupWaves];
  const long n = (long)blockIdx.x * kGroup + threadIdx.x;
  const bool live = n < N;
  const long nc = live ? n : N - 1;                  // a lane past the grid works on the last node and stores nothing
  const long slab = (long)nx * ny;
  const int k = (int)(nc / slab);
  const int j = (int)((nc - k * slab) / nx), i = (int)(nc - k * slab - (long)j * nx);
  unsigned vbits, ibits;
  corner_bits(tsdf, wsum, nc, i, j, k, nx, ny, nz, min_weight, vbits, ibits);
  const unsigned m = live ? edge_mask_of(vbits, ibits) : 0u;
  int nf = 0;
  if (live && i < nx - 1 && j < ny - 1 && k < nz - 1) {
#pragma unroll
    for (int t = 0; t < 6; ++t) {
      unsigned codes;
      int pattern;
      if (tet_pattern(t, vbits, ibits, codes, pattern)) nf += d_cases[0][pattern][0];
    }
  }
  const int nv = __popc(m);
  int tv, tf;
  const int pv = block_scan_int<kGroupWaves>(nv, s_wv, &tv);
  const int pf = block_scan_int<kGroupWaves>(nf, s_wf, &tf);
  if (live) {
    edge_mask[n] = (uint8_t)m;
    vertex_offset[n] = pv;
    face_offset[n] = pf;
  }
  if (threadIdx.x == 0) {
    group_counts[2 * (long)blockIdx.x] = tv;
    group_counts[2 * (long)blockIdx.x + 1] = tf;
  }
}

// The second level: one workgroup walks the groups' counts in chunks of 1024 with a running carry.
__global__ __launch_bounds__(kScanThreads) void mesh_scan_kernel(const int32_t* __restrict__ group_counts, long G,
                                                                 int64_t* __restrict__ group_offsets, int64_t* __restrict__ counts) {
  __shared__ long long s_w[2][kScanWaves];
  const int tid = threadIdx.x, lane = lane_id(), w = tid / kWave;
  long long carry_v = 0, carry_f = 0;
  for (long base = 0; base < G; base += kScanThreads) {
    const long g = base + tid;
    const long long v = g < G ? (long long)group_counts[2 * g] : 0, f = g < G ? (long long)group_counts[2 * g + 1] : 0;
    long long xv = v, xf = f;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const long long yv = __shfl_up(xv, d, kWave), yf = __shfl_up(xf, d, kWave);
      if (lane >= d) {
        xv += yv;
        xf += yf;
      }
    }
    if (lane == kWave - 1) {
      s_w[0][w] = xv;
      s_w[1][w] = xf;
    }
    __syncthreads();
    long long bv = 0, bf = 0, tv = 0, tf = 0;
#pragma unroll
    for (int q = 0; q < kScanWaves; ++q) {
      bv += q < w ? s_w[0][q] : 0;
      bf += q < w ? s_w[1][q] : 0;
      tv += s_w[0][q];
      tf += s_w[1][q];
    }
    if (g < G) {
      group_offsets[2 * g] = (int64_t)(carry_v + bv + xv - v);
      group_offsets[2 * g + 1] = (int64_t)(carry_f + bf + xf - f);
    }
    carry_v += tv;
    carry_f += tf;
    __syncthreads();                                 // s_w is rewritten by the next chunk
  }
  if (tid == 0) {
    counts[0] = (int64_t)carry_v;
    counts[1] = (int64_t)carry_f;
  }
}

// ------------------------------------------------------------------------------------------------------- emission
// the header's gradient of s at the valid node n = (i, j, k) with value s0; false: missing along some axis
__device__ __forceinline__ bool node_gradient(const double* __restrict__ tsdf, const double* __restrict__ wsum, long n, int i, int j,
                                           int k, int nx, int ny, int nz, double min_weight, double h, double s0, double* g) {
  bool has = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int idx = a == 0 ? i : (a == 1 ? j : k), dim = a == 0 ? nx : (a == 1 ? ny : nz);
    const long step = a == 0 ? 1L : (a == 1 ? (long)nx : (long)nx * ny);
    const bool ep = idx + 1 < dim, em = idx > 0;
    double sp, sm;
    const bool plus = node_value(tsdf, wsum, ep ? n + step : n, min_weight, sp) && ep;
    const bool minus = node_value(tsdf, wsum, em ? n - step : n, min_weight, sm) && em;
    has = has && (plus || minus);
    g[a] = plus && minus ? (sp - sm) / (2.0 * h) : (plus ? (sp - s0) / h : (s0 - sm) / h);
  }
  return has;
}

// One lane per node: the vertices of its edges, then the faces of its cell.  No barrier: lanes leave as they finish.
__global__ __launch_bounds__(kGroup) void mesh_emit_kernel(const double* __restrict__ tsdf, const double* __restrict__ wsum,
                                                           const double* __restrict__ rgb_sum, Grid gr, double min_weight,
                                                           const uint8_t* __restrict__ edge_mask,
                                                           const int32_t* __restrict__ vertex_offset,
                                                           const int32_t* __restrict__ face_offset,
                                                           const int64_t* __restrict__ group_offsets, long vcap, long fcap,
                                                           double* __restrict__ out_vertices, float* __restrict__ out_normals,
                                                           float* __restrict__ out_rgb, int32_t* __restrict__ out_faces) {
  const long n = (long)blockIdx.x * kGroup + threadIdx.x;
  if (n >= gr.N) return;
  const int nx = gr.nx, ny = gr.ny, nz = gr.nz;
  const long slab = (long)nx * ny;
  const int k = (int)(n / slab);
  const int j = (int)((n - k * slab) / nx), i = (int)(n - k * slab - (long)j * nx);
  const unsigned m = edge_mask[n];
  if (m != 0u) {
    double sa, ga[3];
    node_value(tsdf, wsum, n, min_weight, sa);
    const bool has_a = node_gradient(tsdf, wsum, n, i, j, k, nx, ny, nz, min_weight, gr.h, sa, ga);
    const double wa = wsum[n];
    const double Xa[3] = {gr.o[0] + gr.h * (double)i, gr.o[1] + gr.h * (double)j, gr.o[2] + gr.h * (double)k};
    long row = (long)group_offsets[2 * (n / kGroup)] + vertex_offset[n];
    for (int e = 0; e < 7; ++e) {
      if (!((m >> e) & 1u)) continue;
      const int c = nib(kEdgeCode, e);
      const int di = c & 1, dj = (c >> 1) & 1, dk = (c >> 2) & 1;
      if (i + di >= nx || j + dj >= ny || k + dk >= nz) continue;   // (a mask of vggv_mesh_count never says so)
      const long b = n + code_offset(c, nx, ny);
      double sb, gb[3];
      node_value(tsdf, wsum, b, min_weight, sb);
      const bool has_b = node_gradient(tsdf, wsum, b, i + di, j + dj, k + dk, nx, ny, nz, min_weight, gr.h, sb, gb);
      const double t = sa / (sa - sb);
      if (row < vcap) {
        const double Xb[3] = {gr.o[0] + gr.h * (double)(i + di), gr.o[1] + gr.h * (double)(j + dj),
                              gr.o[2] + gr.h * (double)(k + dk)};
        double g[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          out_vertices[3 * row + q] = Xa[q] + t * (Xb[q] - Xa[q]);
          g[q] = ga[q] + t * (gb[q] - ga[q]);
        }
        const double len = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
        const bool ok = has_a && has_b && len > 0.0;
#pragma unroll
        for (int q = 0; q < 3; ++q) out_normals[3 * row + q] = ok ? (float)(g[q] / len) : 0.0f;
        if (rgb_sum != nullptr) {
          const double wb = wsum[b];
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            const double ca = rgb_sum[3 * n + q] / wa, cb = rgb_sum[3 * b + q] / wb;
            out_rgb[3 * row + q] = (float)(ca + t * (cb - ca));
          }
        }
      }
      ++row;
    }
  }
  if (!(i < nx - 1 && j < ny - 1 && k < nz - 1)) return;
  unsigned vbits, ibits;
  corner_bits(tsdf, wsum, n, i, j, k, nx, ny, nz, min_weight, vbits, ibits);
  long frow = (long)group_offsets[2 * (n / kGroup) + 1] + face_offset[n];
  for (int t = 0; t < 6; ++t) {
    unsigned codes;
    int pattern;
    if (!tet_pattern(t, vbits, ibits, codes, pattern)) continue;
    const int8_t* cs = d_cases[(kTetOdd >> t) & 1u][pattern];
    const int ntri = cs[0];
    for (int r = 0; r < ntri; ++r) {
      if (frow < fcap) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const int eid = cs[1 + 3 * r + q];
          const int cx = nib(codes, nib(kEdgeLo, eid)), cy = nib(codes, nib(kEdgeHi, eid));
          const long owner = n + code_offset(cx, nx, ny);
          const int e = nib(kCodeEdge, cx ^ cy);
          const long id = (long)group_offsets[2 * (owner / kGroup)] + vertex_offset[owner] +
                          __popc((unsigned)edge_mask[owner] & ((1u << e) - 1u));
          out_faces[3 * frow + q] = (int32_t)id;
        }
      }
      ++frow;
    }
  }
}

// VGG_OK with *N = 0: nothing to do; VGG_OK with *N > 0: go; else the refusal
static int grid_nodes(int nx, int ny, int nz, long* N) {
  *N = 0;
  if (nx < 0 || ny < 0 || nz < 0 || nx == 1 || ny == 1 || nz == 1) return VGG_ERR_INVALID_ARGUMENT;
  if (nx == 0 || ny == 0 || nz == 0) return VGG_OK;
  const long slab = (long)nx * ny;
  if (slab > kMaxNodes || slab * nz > kMaxNodes) return VGG_ERR_UNSUPPORTED;
  *N = slab * nz;
  return VGG_OK;
}

static Grid make_grid(double ox, double oy, double oz, double h, int nx, int ny, int nz, long N) {
  Grid g;
  memset(&g, 0, sizeof(g));
  g.o[0] = ox;
  g.o[1] = oy;
  g.o[2] = oz;
  g.h = h;
  g.nx = nx;
  g.ny = ny;
  g.nz = nz;
  g.N = N;
  return g;
}

}  // namespace vgg

using namespace vgg;

extern "C" {

const char* vggv_build_arch(void) { return "gfx950"; }

int vggv_case_table(int32_t* out) {
  if (!out) return VGG_ERR_INVALID_ARGUMENT;
  for (int s = 0; s < 2; ++s)
    for (int p = 0; p < 16; ++p)
      for (int q = 0; q < 7; ++q) out[(s * 16 + p) * 7 + q] = h_cases[s][p][q];
  return VGG_OK;
}

int vggv_integrate(const float* depth, const float* weights, const float* frames, const double* poses, const double* cams,
                   int num_frames, int height, int width, double origin_x, double origin_y, double origin_z, double voxel,
                   int nx, int ny, int nz, double trunc, double* tsdf_sum, double* weight_sum, double* rgb_sum, void* stream) {
  if (!(trunc > 0.0) || !(voxel > 0.0) || num_frames < 1 || height < 0 || width < 0) return VGG_ERR_INVALID_ARGUMENT;
  long N;
  const int rc = grid_nodes(nx, ny, nz, &N);
  if (rc != VGG_OK) return rc;
  if (N == 0 || height == 0 || width == 0) return VGG_OK;
  if (!depth || !poses || !cams || !tsdf_sum || !weight_sum) return VGG_ERR_INVALID_ARGUMENT;
  if ((long)height * width > (long)INT32_MAX) return VGG_ERR_UNSUPPORTED;
  const Grid g = make_grid(origin_x, origin_y, origin_z, voxel, nx, ny, nz, N);
  for (int first = 0; first < num_frames; first += kMaxViews) {
    const int count = num_frames - first < kMaxViews ? num_frames - first : kMaxViews;
    tsdf_integrate_kernel<<<div_up(N, 256), 256, 0, (hipStream_t)stream>>>(depth, weights, frames, poses, cams, first, count,
                                                                          height, width, g, trunc, tsdf_sum, weight_sum, rgb_sum);
    VGG_LAUNCH_CHECK();
  }
  return VGG_OK;
}

int vggv_mesh_count(const double* tsdf_sum, const double* weight_sum, int nx, int ny, int nz, double min_weight,
                    uint8_t* edge_mask, int32_t* vertex_offset, int32_t* face_offset, int32_t* group_counts,
                    int64_t* group_offsets, int64_t* counts, void* stream) {
  if (!(min_weight > 0.0)) return VGG_ERR_INVALID_ARGUMENT;
  long N;
  const int rc = grid_nodes(nx, ny, nz, &N);
  if (rc != VGG_OK) return rc;
  if (N == 0) return VGG_OK;
  if (!tsdf_sum || !weight_sum || !edge_mask || !vertex_offset || !face_offset || !group_counts || !group_offsets || !counts)
    return VGG_ERR_INVALID_ARGUMENT;
  const int G = div_up(N, kGroup);
  hipStream_t st = (hipStream_t)stream;
  mesh_count_kernel<<<G, kGroup, 0, st>>>(tsdf_sum, weight_sum, nx, ny, nz, N, min_weight, edge_mask, vertex_offset, face_offset,
                                          group_counts);
  VGG_LAUNCH_CHECK();
  mesh_scan_kernel<<<1, kScanThreads, 0, st>>>(group_counts, (long)G, group_offsets, counts);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vggv_mesh_emit(const double* tsdf_sum, const double* weight_sum, const double* rgb_sum, double origin_x, double origin_y,
                   double origin_z, double voxel, int nx, int ny, int nz, double min_weight, const uint8_t* edge_mask,
                   const int32_t* vertex_offset, const int32_t* face_offset, const int64_t* group_offsets,
                   long vertex_capacity, long face_capacity, double* out_vertices, float* out_normals, float* out_rgb,
                   int32_t* out_faces, void* stream) {
  if (!(voxel > 0.0) || !(min_weight > 0.0) || vertex_capacity < 0 || face_capacity < 0) return VGG_ERR_INVALID_ARGUMENT;
  long N;
  const int rc = grid_nodes(nx, ny, nz, &N);
  if (rc != VGG_OK) return rc;
  if (N == 0) return VGG_OK;
  if (!tsdf_sum || !weight_sum || !edge_mask || !vertex_offset || !face_offset || !group_offsets || !out_vertices ||
      !out_normals || !out_faces || (rgb_sum && !out_rgb))
    return VGG_ERR_INVALID_ARGUMENT;
  const Grid g = make_grid(origin_x, origin_y, origin_z, voxel, nx, ny, nz, N);
  mesh_emit_kernel<<<div_up(N, kGroup), kGroup, 0, (hipStream_t)stream>>>(tsdf_sum, weight_sum, rgb_sum, g, min_weight, edge_mask,
                                                                         vertex_offset, face_offset, group_offsets, vertex_capacity,
                                                                         face_capacity, out_vertices, out_normals, out_rgb,
                                                                         out_faces);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

}  // extern "C"
