// The uniform grid of vggsfm_amd_nn.h and the closest point of a triangle, as device helpers: the ONE copy that nn.hip (the
// nearest-neighbour library) and icp/icp.hip (the registration library) walk the grid with.  Parity code: every expression
// stands in the header's order, and a file that includes this is built with -ffp-contract=off (sidelib.mk).
#pragma once
#include <math.h>

#include "../common.hpp"
#include "../mvs/mvs_geometry.hpp"

namespace vgg {

constexpr double kAxisLimit = 1099511627776.0;   // 2^40: beyond it (in cells) a query takes the whole axis

// by-value kernel argument, validated on the host
struct Grid {
  double ox, oy, oz, cell;
  int d0, d1, d2;
};

__device__ __forceinline__ bool finite3(double x, double y, double z) { return x - x == 0.0 && y - y == 0.0 && z - z == 0.0; }

// c_a of the header for the coordinate p, moved by `shift` cells before the clamp (the margin of a query's range)
__device__ __forceinline__ int axis_cell(double p, double o, double cell, int dim, double shift) {
  double t = floor((p - o) / cell) + shift;
  t = fmin(fmax(t, -1.0), (double)dim);              // keeps the conversion defined for infinities; the clamp follows
  return clampi((int)t, dim - 1);
}

// the range of cells of a query on one axis
__device__ __forceinline__ void axis_range(double q, double r, double o, double cell, int dim, int& lo, int& hi) {
  if (fabs(q) < kAxisLimit * cell && r < kAxisLimit * cell) {
    lo = axis_cell(q - r, o, cell, dim, -1.0);
    hi = axis_cell(q + r, o, cell, dim, 1.0);
  } else {
    lo = 0;
    hi = dim - 1;
  }
}

__device__ __forceinline__ double dot3(double x0, double x1, double x2, double y0, double y1, double y2) {
  return ((x0 * y0) + (x1 * y1)) + x2 * y2;
}

struct Triangle {
  double a0, a1, a2, b0, b1, b2, c0, c1, c2;
};

// the vertices of face `f` whose rows lie in [0, V) and differ; false: no vertex is loaded
__device__ __forceinline__ bool face_vertices(const double* __restrict__ vertices, int V, const int32_t* __restrict__ faces, long f,
                                              Triangle& t) {
  const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V || i0 == i1 || i1 == i2 || i0 == i2) return false;
  const double *A = vertices + 3 * (long)i0, *B = vertices + 3 * (long)i1, *C = vertices + 3 * (long)i2;
  t.a0 = A[0]; t.a1 = A[1]; t.a2 = A[2];
  t.b0 = B[0]; t.b1 = B[1]; t.b2 = B[2];
  t.c0 = C[0]; t.c1 = C[1]; t.c2 = C[2];
  return true;
}

// the closest point of the triangle to q: the header's seven regions in the header's order
__device__ __forceinline__ void closest_point(const Triangle& t, double q0, double q1, double q2, double& x0, double& x1, double& x2) {
  const double ab0 = t.b0 - t.a0, ab1 = t.b1 - t.a1, ab2 = t.b2 - t.a2;
  const double ac0 = t.c0 - t.a0, ac1 = t.c1 - t.a1, ac2 = t.c2 - t.a2;
  const double d1 = dot3(ab0, ab1, ab2, q0 - t.a0, q1 - t.a1, q2 - t.a2), d2 = dot3(ac0, ac1, ac2, q0 - t.a0, q1 - t.a1, q2 - t.a2);
  if (d1 <= 0.0 && d2 <= 0.0) {
    x0 = t.a0; x1 = t.a1; x2 = t.a2;
    return;
  }
  const double d3 = dot3(ab0, ab1, ab2, q0 - t.b0, q1 - t.b1, q2 - t.b2), d4 = dot3(ac0, ac1, ac2, q0 - t.b0, q1 - t.b1, q2 - t.b2);
  if (d3 >= 0.0 && d4 <= d3) {
    x0 = t.b0; x1 = t.b1; x2 = t.b2;
    return;
  }
  const double vc = (d1 * d4) - (d3 * d2);
  if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
    const double v = d1 / (d1 - d3);
    x0 = t.a0 + v * ab0; x1 = t.a1 + v * ab1; x2 = t.a2 + v * ab2;
    return;
  }
  const double d5 = dot3(ab0, ab1, ab2, q0 - t.c0, q1 - t.c1, q2 - t.c2), d6 = dot3(ac0, ac1, ac2, q0 - t.c0, q1 - t.c1, q2 - t.c2);
  if (d6 >= 0.0 && d5 <= d6) {
    x0 = t.c0; x1 = t.c1; x2 = t.c2;
    return;
  }
  const double vb = (d5 * d2) - (d1 * d6);
  if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
    const double w = d2 / (d2 - d6);
    x0 = t.a0 + w * ac0; x1 = t.a1 + w * ac1; x2 = t.a2 + w * ac2;
    return;
  }
  const double va = (d3 * d6) - (d5 * d4), e = d4 - d3, f = d5 - d6;
  if (va <= 0.0 && e >= 0.0 && f >= 0.0) {
    const double w = e / (e + f);
    x0 = t.b0 + w * (t.c0 - t.b0); x1 = t.b1 + w * (t.c1 - t.b1); x2 = t.b2 + w * (t.c2 - t.b2);
    return;
  }
  const double den = 1.0 / ((va + vb) + vc), v = vb * den, w = vc * den;
  x0 = (t.a0 + ab0 * v) + ac0 * w; x1 = (t.a1 + ab1 * v) + ac1 * w; x2 = (t.a2 + ab2 * v) + ac2 * w;
}

// origin, cell and dims as the entries take them -> the kernel argument; false: refused (vggsfm_amd_nn.h)
static inline bool grid_argument(double ox, double oy, double oz, double cell, int d0, int d1, int d2, long max_cells, Grid& g) {
  if (!(cell > 0.0) || d0 < 1 || d1 < 1 || d2 < 1) return false;
  if ((long)d0 > max_cells || (long)d0 * d1 > max_cells || (long)d0 * d1 * d2 > max_cells) return false;
  g = Grid{ox, oy, oz, cell, d0, d1, d2};
  return true;
}

}  // namespace vgg
