// Nearest point and nearest triangle on a uniform grid, and the statistics of such distances, for gfx950: the entries of
// vggsfm_amd_nn.h.  A parity file: built with -ffp-contract=off, every expression in the header's order
// (tests/nearest_cases.py restates it in NumPy over all pairs, with no grid).
#include <math.h>

#include "nn_grid.hpp"
#include "vggsfm_amd_nn.h"

namespace vgg {

struct Thresholds {
  double tau[VGGN_MAX_THRESHOLDS];
  int count;
};

// --------------------------------------------------------------------------------------------------------- the grid
__global__ __launch_bounds__(256) void point_cells_kernel(const double* __restrict__ points, int n, Grid g, int32_t* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
  int id = -1;
  if (finite3(x, y, z)) {
    const int c0 = axis_cell(x, g.ox, g.cell, g.d0, 0.0), c1 = axis_cell(y, g.oy, g.cell, g.d1, 0.0),
              c2 = axis_cell(z, g.oz, g.cell, g.d2, 0.0);
    id = (c2 * g.d1 + c1) * g.d0 + c0;               // < 2^25
  }
  out[i] = id;
}

__global__ __launch_bounds__(256) void gather_points_kernel(const double* __restrict__ points, const int32_t* __restrict__ order, int n,
                                                            double* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int r = order[i];
  const bool ok = r >= 0 && r < n;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[3 * i + c] = ok ? points[3 * (long)r + c] : NAN;
}

__global__ __launch_bounds__(256) void cell_start_kernel(const int32_t* __restrict__ sorted_cell, int n, int num_cells,
                                                         int32_t* __restrict__ cell_start) {
  const long c = (long)blockIdx.x * 256 + threadIdx.x;
  if (c > num_cells) return;
  int lo = 0, hi = n;                                // the first position whose id is >= c
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (sorted_cell[mid] < (int)c) lo = mid + 1;
    else hi = mid;
  }
  cell_start[c] = lo;
}

// ---------------------------------------------------------------------------------------------------- nearest point
// One lane per query, the queries in the order of `visit`.  The rows of cells of the range are contiguous in the sorted
// arrays, so a lane makes one pass per (c2, c1).  No LDS, no atomic.
__global__ __launch_bounds__(256) void nearest_point_kernel(const double* __restrict__ grid_points, const int32_t* __restrict__ grid_index,
                                                            const int32_t* __restrict__ cell_start, int n, Grid g,
                                                            const double* __restrict__ queries, const int32_t* __restrict__ visit,
                                                            int m, double r, double r2, int exclude_self,
                                                            int32_t* __restrict__ out_index, double* __restrict__ out_dist2,
                                                            int32_t* __restrict__ out_count) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const int qi = visit[j];
  if (qi < 0 || qi >= m) return;
  const double q0 = queries[3 * (long)qi], q1 = queries[3 * (long)qi + 1], q2 = queries[3 * (long)qi + 2];
  double best = INFINITY;
  int bi = -1, count = 0;
  if (n > 0 && finite3(q0, q1, q2)) {
    int lo0, hi0, lo1, hi1, lo2, hi2;
    axis_range(q0, r, g.ox, g.cell, g.d0, lo0, hi0);
    axis_range(q1, r, g.oy, g.cell, g.d1, lo1, hi1);
    axis_range(q2, r, g.oz, g.cell, g.d2, lo2, hi2);
    for (int c2 = lo2; c2 <= hi2; ++c2) {
      for (int c1 = lo1; c1 <= hi1; ++c1) {
        const long row = ((long)c2 * g.d1 + c1) * g.d0;
        const int s = max(cell_start[row + lo0], 0), e = min(cell_start[row + hi0 + 1], n);
        for (int k = s; k < e; ++k) {
          const double dx = q0 - grid_points[3 * (long)k], dy = q1 - grid_points[3 * (long)k + 1],
                       dz = q2 - grid_points[3 * (long)k + 2];
          const double d2 = ((dx * dx) + (dy * dy)) + dz * dz;
          if (!(d2 <= r2)) continue;
          const int idx = grid_index[k];
          if (exclude_self && idx == qi) continue;
          ++count;
          if (bi < 0 || d2 < best || (d2 == best && idx < bi)) {
            best = d2;
            bi = idx;
          }
        }
      }
    }
  }
  out_index[qi] = bi;
  out_dist2[qi] = bi < 0 ? INFINITY : best;
  if (out_count != nullptr) out_count[qi] = count;
}

// ------------------------------------------------------------------------------------------------------- triangles
// the header's validity of a face and the box of cells it is registered in
__device__ __forceinline__ bool face_box(const double* __restrict__ vertices, int V, const int32_t* __restrict__ faces, long f,
                                         const Grid& g, int* lo, int* hi) {
  Triangle t;
  if (!face_vertices(vertices, V, faces, f, t)) return false;
  if (!(finite3(t.a0, t.a1, t.a2) && finite3(t.b0, t.b1, t.b2) && finite3(t.c0, t.c1, t.c2))) return false;
  const double ab0 = t.b0 - t.a0, ab1 = t.b1 - t.a1, ab2 = t.b2 - t.a2, ac0 = t.c0 - t.a0, ac1 = t.c1 - t.a1, ac2 = t.c2 - t.a2;
  const double n0 = ab1 * ac2 - ab2 * ac1, n1 = ab2 * ac0 - ab0 * ac2, n2 = ab0 * ac1 - ab1 * ac0;
  if (!(((n0 * n0) + (n1 * n1)) + n2 * n2 > 0.0)) return false;
  lo[0] = axis_cell(fmin(fmin(t.a0, t.b0), t.c0), g.ox, g.cell, g.d0, 0.0);
  hi[0] = axis_cell(fmax(fmax(t.a0, t.b0), t.c0), g.ox, g.cell, g.d0, 0.0);
  lo[1] = axis_cell(fmin(fmin(t.a1, t.b1), t.c1), g.oy, g.cell, g.d1, 0.0);
  hi[1] = axis_cell(fmax(fmax(t.a1, t.b1), t.c1), g.oy, g.cell, g.d1, 0.0);
  lo[2] = axis_cell(fmin(fmin(t.a2, t.b2), t.c2), g.oz, g.cell, g.d2, 0.0);
  hi[2] = axis_cell(fmax(fmax(t.a2, t.b2), t.c2), g.oz, g.cell, g.d2, 0.0);
  return true;
}

__global__ __launch_bounds__(256) void face_cell_counts_kernel(const double* __restrict__ vertices, int V, const int32_t* __restrict__ faces,
                                                               int F, Grid g, int32_t* __restrict__ out) {
  const long f = (long)blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  int lo[3], hi[3];
  const bool ok = face_box(vertices, V, faces, f, g, lo, hi);
  out[f] = ok ? (hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1) : 0;      // <= 2^25
}

__global__ __launch_bounds__(256) void face_cell_pairs_kernel(const double* __restrict__ vertices, int V, const int32_t* __restrict__ faces,
                                                              int F, Grid g, const int64_t* __restrict__ offset, long num_pairs,
                                                              int32_t* __restrict__ pair_cell, int32_t* __restrict__ pair_face) {
  const long f = (long)blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  int lo[3], hi[3];
  if (!face_box(vertices, V, faces, f, g, lo, hi)) return;
  const long count = (long)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1);
  long o = offset[f];
  if (o < 0 || o > num_pairs - count) return;        // the pairs of this face would not fit: none is written
  for (int c2 = lo[2]; c2 <= hi[2]; ++c2)
    for (int c1 = lo[1]; c1 <= hi[1]; ++c1)
      for (int c0 = lo[0]; c0 <= hi[0]; ++c0) {
        pair_cell[o] = (c2 * g.d1 + c1) * g.d0 + c0;
        pair_face[o] = (int32_t)f;
        ++o;
      }
}

// One lane per query, as for points; a face registered in several cells of the range is met again and changes nothing.
__global__ __launch_bounds__(256) void nearest_face_kernel(const double* __restrict__ vertices, int V, const int32_t* __restrict__ faces,
                                                           int F, const int32_t* __restrict__ cell_faces,
                                                           const int32_t* __restrict__ cell_start, int num_pairs, Grid g,
                                                           const double* __restrict__ queries, const int32_t* __restrict__ visit,
                                                           int m, double r, double r2, int32_t* __restrict__ out_face,
                                                           double* __restrict__ out_dist2, double* __restrict__ out_closest) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  const int qi = visit[j];
  if (qi < 0 || qi >= m) return;
  const double q0 = queries[3 * (long)qi], q1 = queries[3 * (long)qi + 1], q2 = queries[3 * (long)qi + 2];
  double best = INFINITY, b0 = NAN, b1 = NAN, b2 = NAN;
  int bf = -1;
  if (num_pairs > 0 && F > 0 && finite3(q0, q1, q2)) {
    int lo0, hi0, lo1, hi1, lo2, hi2;
    axis_range(q0, r, g.ox, g.cell, g.d0, lo0, hi0);
    axis_range(q1, r, g.oy, g.cell, g.d1, lo1, hi1);
    axis_range(q2, r, g.oz, g.cell, g.d2, lo2, hi2);
    for (int c2 = lo2; c2 <= hi2; ++c2) {
      for (int c1 = lo1; c1 <= hi1; ++c1) {
        const long row = ((long)c2 * g.d1 + c1) * g.d0;
        const int s = max(cell_start[row + lo0], 0), e = min(cell_start[row + hi0 + 1], num_pairs);
        for (int k = s; k < e; ++k) {
          const int f = cell_faces[k];
          Triangle t;
          if (f < 0 || f >= F || f == bf || !face_vertices(vertices, V, faces, f, t)) continue;
          double x0, x1, x2;
          closest_point(t, q0, q1, q2, x0, x1, x2);
          const double dx = q0 - x0, dy = q1 - x1, dz = q2 - x2;
          const double d2 = ((dx * dx) + (dy * dy)) + dz * dz;
          if (!(d2 <= r2)) continue;
          if (bf < 0 || d2 < best || (d2 == best && f < bf)) {
            best = d2;
            bf = f;
            b0 = x0; b1 = x1; b2 = x2;
          }
        }
      }
    }
  }
  out_face[qi] = bf;
  out_dist2[qi] = bf < 0 ? INFINITY : best;
  if (out_closest != nullptr) {
    out_closest[3 * (long)qi] = b0;
    out_closest[3 * (long)qi + 1] = b1;
    out_closest[3 * (long)qi + 2] = b2;
  }
}

// ------------------------------------------------------------------------------------------------------ statistics
// VGGN_STATS_GROUPS workgroups of one wavefront; every lane reaches the butterflies (no early return).
__global__ __launch_bounds__(64) void stats_partial_kernel(const double* __restrict__ dist2, int m, Thresholds th, double* __restrict__ ws) {
  const int g = blockIdx.x, lane = threadIdx.x;
  double sum_d = 0.0, sum_d2 = 0.0;
  int found = 0, below[VGGN_MAX_THRESHOLDS];
#pragma unroll
  for (int k = 0; k < VGGN_MAX_THRESHOLDS; ++k) below[k] = 0;
  for (long i = 64L * g + lane; i < m; i += 64L * VGGN_STATS_GROUPS) {
    const double d2 = dist2[i];
    if (d2 - d2 == 0.0) {
      const double d = sqrt(d2);
      sum_d = sum_d + d;
      sum_d2 = sum_d2 + d2;
      ++found;
#pragma unroll
      for (int k = 0; k < VGGN_MAX_THRESHOLDS; ++k) below[k] += (k < th.count && d < th.tau[k]) ? 1 : 0;
    }
  }
  sum_d = wave_sum(sum_d);
  sum_d2 = wave_sum(sum_d2);
  found = wave_sum_i(found);
#pragma unroll
  for (int k = 0; k < VGGN_MAX_THRESHOLDS; ++k) below[k] = wave_sum_i(below[k]);
  if (lane == 0) {
    double* w = ws + (long)g * VGGN_STATS_WORDS;
    long long* wi = (long long*)w;
    w[0] = sum_d;
    w[1] = sum_d2;
    wi[2] = found;
#pragma unroll
    for (int k = 0; k < VGGN_MAX_THRESHOLDS; ++k) wi[3 + k] = below[k];
    wi[11] = 0;
  }
}

// lane w adds word w of the partials in ascending group order
__global__ __launch_bounds__(64) void stats_final_kernel(const double* __restrict__ ws, int num_thresholds, int64_t* __restrict__ out_counts,
                                                         double* __restrict__ out_sums) {
  const int w = threadIdx.x;
  if (w < 2) {
    double s = 0.0;
    for (int g = 0; g < VGGN_STATS_GROUPS; ++g) s = s + ws[(long)g * VGGN_STATS_WORDS + w];
    out_sums[w] = s;
  } else if (w < 3 + num_thresholds) {
    const long long* wi = (const long long*)ws;
    long long s = 0;
    for (int g = 0; g < VGGN_STATS_GROUPS; ++g) s += wi[(long)g * VGGN_STATS_WORDS + w];
    out_counts[w - 2] = s;
  }
}

static bool make_grid(double ox, double oy, double oz, double cell, int d0, int d1, int d2, Grid& g) {
  return grid_argument(ox, oy, oz, cell, d0, d1, d2, VGGN_MAX_CELLS, g);
}

}  // namespace vgg

using namespace vgg;

extern "C" {

const char* vggn_build_arch(void) { return "gfx950"; }

int vggn_point_cells(const double* points, int n, double ox, double oy, double oz, double cell, int d0, int d1, int d2,
                     int32_t* out_cell, void* stream) {
  Grid g;
  if (!make_grid(ox, oy, oz, cell, d0, d1, d2, g) || n < 0) return VGG_ERR_INVALID_ARGUMENT;
  if (n == 0) return VGG_OK;
  if (!points || !out_cell) return VGG_ERR_INVALID_ARGUMENT;
  point_cells_kernel<<<div_up(n, 256), 256, 0, (hipStream_t)stream>>>(points, n, g, out_cell);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vggn_gather_points(const double* points, const int32_t* order, int n, double* out_points, void* stream) {
  if (n < 0) return VGG_ERR_INVALID_ARGUMENT;
  if (n == 0) return VGG_OK;
  if (!points || !order || !out_points) return VGG_ERR_INVALID_ARGUMENT;
  gather_points_kernel<<<div_up(n, 256), 256, 0, (hipStream_t)stream>>>(points, order, n, out_points);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vggn_cell_start(const int32_t* sorted_cell, int n, int num_cells, int32_t* cell_start, void* stream) {
  if (n < 0 || num_cells < 1 || num_cells > VGGN_MAX_CELLS) return VGG_ERR_INVALID_ARGUMENT;
  if (!cell_start || (n > 0 && !sorted_cell)) return VGG_ERR_INVALID_ARGUMENT;
  cell_start_kernel<<<div_up((long)num_cells + 1, 256), 256, 0, (hipStream_t)stream>>>(sorted_cell, n, num_cells, cell_start);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vggn_nearest_point(const double* grid_points, const int32_t* grid_index, const int32_t* cell_start, int n, double ox,
                       double oy, double oz, double cell, int d0, int d1, int d2, const double* queries,
                       const int32_t* visit, int m, double max_dist, double r2, int exclude_self, int32_t* out_index,
                       double* out_dist2, int32_t* out_count, void* stream) {
  Grid g;
  if (!make_grid(ox, oy, oz, cell, d0, d1, d2, g) || !(max_dist > 0.0) || !(r2 >= 0.0) || n < 0 || m < 0)
    return VGG_ERR_INVALID_ARGUMENT;
  if (m == 0) return VGG_OK;
  if (!queries || !visit || !out_index || !out_dist2 || (n > 0 && (!grid_points || !grid_index || !cell_start)))
    return VGG_ERR_INVALID_ARGUMENT;
  nearest_point_kernel<<<div_up(m, 256), 256, 0, (hipStream_t)stream>>>(grid_points, grid_index, cell_start, n, g, queries, visit, m,
                                                                        max_dist, r2, exclude_self, out_index, out_dist2, out_count);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vggn_face_cell_counts(const double* vertices, int num_vertices, const int32_t* faces, int num_faces, double ox, double oy,
                          double oz, double cell, int d0, int d1, int d2, int32_t* out_count, void* stream) {
  Grid g;
  if (!make_grid(ox, oy, oz, cell, d0, d1, d2, g) || num_vertices < 0 || num_faces < 0) return VGG_ERR_INVALID_ARGUMENT;
  if (num_faces == 0) return VGG_OK;
  if (!faces || !out_count || (num_vertices > 0 && !vertices)) return VGG_ERR_INVALID_ARGUMENT;
  face_cell_counts_kernel<<<div_up(num_faces, 256), 256, 0, (hipStream_t)stream>>>(vertices, num_vertices, faces, num_faces, g,
                                                                                   out_count);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vggn_face_cell_pairs(const double* vertices, int num_vertices, const int32_t* faces, int num_faces, double ox, double oy,
                         double oz, double cell, int d0, int d1, int d2, const int64_t* offset, long num_pairs,
                         int32_t* pair_cell, int32_t* pair_face, void* stream) {
  Grid g;
  if (!make_grid(ox, oy, oz, cell, d0, d1, d2, g) || num_vertices < 0 || num_faces < 0 || num_pairs < 0 ||
      num_pairs > (long)INT32_MAX)
    return VGG_ERR_INVALID_ARGUMENT;
  if (num_faces == 0 || num_pairs == 0) return VGG_OK;
  if (!faces || !offset || !pair_cell || !pair_face || (num_vertices > 0 && !vertices)) return VGG_ERR_INVALID_ARGUMENT;
  face_cell_pairs_kernel<<<div_up(num_faces, 256), 256, 0, (hipStream_t)stream>>>(vertices, num_vertices, faces, num_faces, g, offset,
                                                                                  num_pairs, pair_cell, pair_face);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vggn_nearest_face(const double* vertices, int num_vertices, const int32_t* faces, int num_faces, const int32_t* cell_faces,
                      const int32_t* cell_start, int num_pairs, double ox, double oy, double oz, double cell, int d0, int d1,
                      int d2, const double* queries, const int32_t* visit, int m, double max_dist, double r2,
                      int32_t* out_face, double* out_dist2, double* out_closest, void* stream) {
  Grid g;
  if (!make_grid(ox, oy, oz, cell, d0, d1, d2, g) || !(max_dist > 0.0) || !(r2 >= 0.0) || num_vertices < 0 || num_faces < 0 ||
      num_pairs < 0 || m < 0)
    return VGG_ERR_INVALID_ARGUMENT;
  if (m == 0) return VGG_OK;
  const bool work = num_faces > 0 && num_pairs > 0;
  if (!queries || !visit || !out_face || !out_dist2 || (work && (!vertices || !faces || !cell_faces || !cell_start)))
    return VGG_ERR_INVALID_ARGUMENT;
  nearest_face_kernel<<<div_up(m, 256), 256, 0, (hipStream_t)stream>>>(vertices, num_vertices, faces, num_faces, cell_faces, cell_start,
                                                                       num_pairs, g, queries, visit, m, max_dist, r2, out_face,
                                                                       out_dist2, out_closest);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vggn_distance_stats(const double* dist2, int m, const double* thresholds, int num_thresholds, int64_t* out_counts,
                        double* out_sums, void* workspace, void* stream) {
  if (m < 0 || num_thresholds < 0 || num_thresholds > VGGN_MAX_THRESHOLDS || (num_thresholds > 0 && !thresholds))
    return VGG_ERR_INVALID_ARGUMENT;
  if (!out_counts || !out_sums || !workspace || (m > 0 && !dist2)) return VGG_ERR_INVALID_ARGUMENT;
  Thresholds th;
  memset(&th, 0, sizeof(th));
  th.count = num_thresholds;
  for (int k = 0; k < num_thresholds; ++k) th.tau[k] = thresholds[k];
  stats_partial_kernel<<<VGGN_STATS_GROUPS, 64, 0, (hipStream_t)stream>>>(dist2, m, th, (double*)workspace);
  VGG_LAUNCH_CHECK();
  stats_final_kernel<<<1, 64, 0, (hipStream_t)stream>>>((const double*)workspace, num_thresholds, out_counts, out_sums);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

}  // extern "C"
