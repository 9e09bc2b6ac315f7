// The support of a RANSAC hypothesis, as every robust estimator of the library that shares the rule counts and ranks it.
#pragma once
#include "common.hpp"

namespace vgg {

// squared residual of X under the 3x4 pose P on the normalised plane; in support if in front of the camera and within thr_sq
__device__ __forceinline__ bool point_error(const double* __restrict__ P, double X0, double X1, double X2, double u, double w,
                                            double thr_sq, double& e) {
  const double px = ((P[0] * X0 + P[1] * X1) + P[2] * X2) + P[3];
  const double py = ((P[4] * X0 + P[5] * X1) + P[6] * X2) + P[7];
  const double pz = ((P[8] * X0 + P[9] * X1) + P[10] * X2) + P[11];
  const bool front = pz > 1e-12;
  const double zs = front ? pz : 1.0;
  const double ex = px / zs - u, ey = py / zs - w;
  e = ex * ex + ey * ey;
  return front && e <= thr_sq;
}

// ranks (count, sum, index): more inliers, then the smaller residual sum, then the lower index: a total order
__device__ __forceinline__ bool ranks_before(int c1, double s1, int i1, int c2, double s2, int i2) {
  if (c1 != c2) return c1 > c2;
  if (s1 != s2) return s1 < s2;
  return i1 < i2;
}

}  // namespace vgg
