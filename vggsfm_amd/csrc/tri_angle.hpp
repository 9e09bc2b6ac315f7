// The triangulation angle of two views at a point, from squared lengths, as the reference computes it, and the projection
// centres it is measured between.
#pragma once
#include "common.hpp"

namespace vgg {

constexpr double kPi = 3.141592653589793;

// projection centre -R^T t of the 3x4 pose P (triangulation_helpers.py:531)
__device__ __forceinline__ void camera_centre(const double* __restrict__ P, double* __restrict__ out) {
  out[0] = -(P[0] * P[3] + P[4] * P[7] + P[8] * P[11]);
  out[1] = -(P[1] * P[3] + P[5] * P[7] + P[9] * P[11]);
  out[2] = -(P[2] * P[3] + P[6] * P[7] + P[10] * P[11]);
}

__device__ __forceinline__ double sqnorm3(double a, double b, double c) {
  const double n = sqrt(a * a + b * b + c * c);   // the reference squares a norm: (x).norm(dim=-1) ** 2
  return n * n;
}

// law of cosines on (norm)^2 values, min(theta, pi - theta), degrees -- triangulation_helpers.py:503-519 and 568-586
__device__ __forceinline__ double tri_angle_deg(double r1, double r2, double b) {
  double den = 2.0 * sqrt(r1 * r2);
  double nom = r1 + r2 - b;
  if (den <= 1e-12) { nom = 1.0; den = 1.0; }
  double c = nom / den;
  c = fmin(fmax(c, -1.0), 1.0);
  double th = fabs(acos(c));
  th = fmin(th, kPi - th);
  return th * (180.0 / kPi);
}

}  // namespace vgg
