// Essential matrices by the 5-point algorithm with LO-RANSAC -- vggsfm/two_view_geo/essential.py:111-488
// (estimate_essential, run_5point, null_to_Nister_solution).  DESIGN.md section 16.
//
// float64, no FMA contraction (-ffp-contract=off), no transcendental functions, every sum in a fixed order.
//
//   emat5_kernel        a group of 16 lanes per (pair, 5-point sample), four samples per wavefront
//   emat_gram_kernel    one workgroup per (pair, selected hypothesis) or per point set: X^T X over the inliers (recomputed
//                       on the fly) or over all weighted rows, fixed-order reductions, then the first wavefront solves
//   two_view_score_kernel  (two_view.hpp, shared with fundamental.hip) with one threshold per pair
// Both solvers end in five_point_from_gram(): the 16 lanes of a group hold the 9x9 matrix X^T X, one row per lane.
//   1  cyclic Jacobi (lane = row); the eigenvectors of the four smallest eigenvalues span E = x N0 + y N1 + z N2 + N3
//   2  lane r < 9 expands entry r of 2 E E^T E - tr(E E^T) E, lane 9 expands det E: ten cubics in (x, y, z), 20 monomials
//   3  Gauss-Jordan on the first ten columns with partial pivoting: one row per lane, the pivot row broadcast by shuffles
//   4  rows (x^2 z, x^2), (y^2 z, y^2), (x y z, x y) give B(z) [x y 1]^T = 0 (Nister 2004); det B(z) has degree 10
//   5  lane s < 10 looks for the (s+1)-th real root: bisection on the Sturm sign-variation count, Newton polish
//   6  [x y 1] is the cross product of two rows of B(z)
//   7  a fixed number of Gauss-Newton steps on the ten constraints polish the coefficients; E is scaled to unit Frobenius
//      norm and transposed
#include "common.hpp"
#include "jacobi.hpp"
#include "two_view.hpp"
#include "../../include/vggsfm_amd_essential.h"

namespace vgg {

constexpr int kGroup = 16;           // lanes per 5-point problem
constexpr int kSturmSteps = 64;      // bisections on the sign-variation count
constexpr int kNewtonSteps = 3;
constexpr int kPolishSteps = 4;      // Gauss-Newton steps on the constraints
constexpr double kRootResidual = 1e-6;   // |p(z)| <= kRootResidual * sum |c_d z^d| or the slot is flagged 0

// ------------------------------------------------------------------------------------------------ polynomials
// variables 0..3 = x, y, z, 1.  Degree 2: the ten products v_i v_j (i <= j) in lexicographic order.  Degree 3: Nister's
// column order  x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
__host__ __device__ constexpr int idx2(int i, int j) {
  return (i == 0 ? 0 : (i == 1 ? 4 : (i == 2 ? 7 : 9))) + (j - i);
}
__host__ __device__ constexpr int col3(int i, int j, int k) {      // i <= j <= k
  const int key = i * 16 + j * 4 + k;
  return key == 0 ? 0 : key == 21 ? 1 : key == 1 ? 2 : key == 5 ? 3 : key == 2 ? 4 : key == 3 ? 5 : key == 22 ? 6
       : key == 23 ? 7 : key == 6 ? 8 : key == 7 ? 9 : key == 10 ? 10 : key == 11 ? 11 : key == 15 ? 12 : key == 26 ? 13
       : key == 27 ? 14 : key == 31 ? 15 : key == 42 ? 16 : key == 43 ? 17 : key == 47 ? 18 : 19;
}
__host__ __device__ constexpr int col3_any(int a, int b, int c) {  // (a <= b), c anywhere
  return c <= a ? col3(c, a, b) : (c <= b ? col3(a, c, b) : col3(a, b, c));
}
// out (degree 2) += sgn * a * b (degree 1 each)
__device__ __forceinline__ void mul11_acc(double* out, const double* a, const double* b, double sgn) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) out[i <= j ? idx2(i, j) : idx2(j, i)] = out[i <= j ? idx2(i, j) : idx2(j, i)] + sgn * (a[i] * b[j]);
}
// out (degree 3, column order) += a (degree 2) * b (degree 1)
__device__ __forceinline__ void mul21_acc(double* out, const double* a, const double* b) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = i; j < 4; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) out[col3_any(i, j, k)] = out[col3_any(i, j, k)] + a[idx2(i, j)] * b[k];
}
__device__ __forceinline__ double sel3(int i, double a, double b, double c) { return i == 0 ? a : (i == 1 ? b : c); }
__device__ __forceinline__ double gshfl(double v, int src) { return __shfl(v, src, kGroup); }

// c (degree na + nb) = a * b, ascending powers, terms added in ascending order of the index of a
template <int NA, int NB>
__device__ __forceinline__ void conv(const double* a, const double* b, double* c) {
#pragma unroll
  for (int d = 0; d <= NA + NB; ++d) {
    double s = 0.0;
    bool first = true;
#pragma unroll
    for (int i = 0; i <= NA; ++i) {
      if (d - i >= 0 && d - i <= NB) { s = first ? a[i] * b[d - i] : s + a[i] * b[d - i]; first = false; }
    }
    c[d] = s;
  }
}

// Sturm chain of p (degree 10, ascending powers): P0 = p, P1 = p', P_{k+1} = -rem(P_{k-1}, P_k) rescaled by a positive
// factor; P_k (k >= 2, degree 10 - k) is kept by its coefficients and evaluated by Horner -- the three-term recurrence
// of the quotients would cancel x^2 worth of digits per step.  The degrees are taken to drop by one each step; where they
// do not, a division by zero makes the counts garbage, and the candidates built from them fail their own checks.
struct Sturm {
  double c[11];
  double P[9][9];      // P[k - 2][0 .. 10 - k]
};
__device__ __forceinline__ void sturm_build(Sturm& S) {
  double p[11], d[11], r[11];
#pragma unroll
  for (int i = 0; i < 11; ++i) { p[i] = S.c[i]; d[i] = (i < 10) ? (double)(i + 1) * S.c[i + 1] : 0.0; r[i] = 0.0; }
#pragma unroll
  for (int k = 1; k <= 9; ++k) {
    const int n = 11 - k;                       // degree of p; d has degree n - 1
    const double qa = p[n] / d[n - 1];
    const double qb = (p[n - 1] - qa * (n >= 2 ? d[n - 2] : 0.0)) / d[n - 1];
    double mx = 0.0;
#pragma unroll
    for (int i = 0; i <= 8; ++i) {
      if (i <= n - 2) {
        const double v = (qb * d[i] + (i >= 1 ? qa * d[i - 1] : 0.0)) - p[i];      // -(p - q d)
        r[i] = v;
        mx = fmax(mx, fabs(v));
      }
    }
    const double sc = 1.0 / mx;
#pragma unroll
    for (int i = 0; i <= 9; ++i) {
      p[i] = d[i];
      d[i] = (i <= n - 2) ? r[i] * sc : 0.0;
    }
#pragma unroll
    for (int i = 0; i <= 8; ++i) S.P[k - 1][i] = d[i];
  }
}
__device__ inline double poly10(const double* c, double x) {
  double f = c[10];
#pragma unroll
  for (int i = 9; i >= 0; --i) f = f * x + c[i];
  return f;
}
__device__ inline double dpoly10(const double* c, double x) {
  double f = 10.0 * c[10];
#pragma unroll
  for (int i = 9; i >= 1; --i) f = f * x + (double)i * c[i];
  return f;
}
// sign variations of the chain at x (zeros skipped)
__device__ __forceinline__ int sturm_variations(const Sturm& S, double x) {
  const double a = poly10(S.c, x);
  int last = (a > 0.0) - (a < 0.0), var = 0;
#pragma unroll
  for (int k = 1; k <= 10; ++k) {
    double b;
    if (k == 1) {
      b = dpoly10(S.c, x);
    } else {
      b = S.P[k - 2][10 - k];
#pragma unroll
      for (int i = 9 - k; i >= 0; --i) b = b * x + S.P[k - 2][i];
    }
    const int sg = (b > 0.0) - (b < 0.0);
    if (sg != 0) { var += (last != 0 && sg != last) ? 1 : 0; last = sg; }
  }
  return var;
}

// ------------------------------------------------------------------------------------------------ 3x3 helpers
__device__ __forceinline__ void mat3_abt(const double* A, const double* B, double* C) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[3 * j] + A[3 * i + 1] * B[3 * j + 1]) + A[3 * i + 2] * B[3 * j + 2];
}
__device__ __forceinline__ void mat3_atb(const double* A, const double* B, double* C) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[i] * B[j] + A[3 + i] * B[3 + j]) + A[6 + i] * B[6 + j];
}
__device__ __forceinline__ void cofactors(const double* E, double* c) {
  c[0] = E[4] * E[8] - E[5] * E[7]; c[1] = E[5] * E[6] - E[3] * E[8]; c[2] = E[3] * E[7] - E[4] * E[6];
  c[3] = E[2] * E[7] - E[1] * E[8]; c[4] = E[0] * E[8] - E[2] * E[6]; c[5] = E[1] * E[6] - E[0] * E[7];
  c[6] = E[1] * E[5] - E[2] * E[4]; c[7] = E[2] * E[3] - E[0] * E[5]; c[8] = E[0] * E[4] - E[1] * E[3];
}
// M = k0 N0 + k1 N1 + k2 N2 + k3 N3
__device__ __forceinline__ void combine(const double (*Nb)[9], const double* k, double* M) {
#pragma unroll
  for (int q = 0; q < 9; ++q) M[q] = ((k[0] * Nb[0][q] + k[1] * Nb[1][q]) + k[2] * Nb[2][q]) + k[3] * Nb[3][q];
}
// r = [det E, 2 E E^T E - tr(E E^T) E]; returns |r|^2
__device__ __forceinline__ double constraint_residual(const double* E, double* r) {
  double EEt[9], T[9], cof[9];
  mat3_abt(E, E, EEt);
  mat3_ab(EEt, E, T);
  cofactors(E, cof);
  const double tr = (EEt[0] + EEt[4]) + EEt[8];
  r[0] = (E[0] * cof[0] + E[1] * cof[1]) + E[2] * cof[2];
  double s = r[0] * r[0];
#pragma unroll
  for (int q = 0; q < 9; ++q) { r[1 + q] = 2.0 * T[q] - tr * E[q]; s = s + r[1 + q] * r[1 + q]; }
  return s;
}

// ------------------------------------------------------------------------------------------------ the shared solve
// Called by all lanes of a wavefront; g = lane within its group of 16.  a[9]: row g of X^T X (lanes g >= 9 pass a copy of
// row 0 and are never read); overwritten.  Lane g < 10 returns candidate slot g in E (p2^T E p1 = 0, unit Frobenius norm).
__device__ __forceinline__ void five_point_from_gram(double* a, int g, double* E, bool& valid) {
  // 1 -- cyclic Jacobi, lane = row of A and of V (as in fmat8_kernel)
  double v[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) v[j] = (j == g) ? 1.0 : 0.0;
  jacobi_rows<9, kGroup, kSweeps9>(a, v, g);
  // the four smallest eigenvalues; nb[k] = component g of basis vector k, N3 the smallest
  double nb[4];
  smallest_by_rank<9, 4, kGroup, true>(a, v, nb);
  // 2 -- the ten cubic constraints, one per lane
  double row[20];
#pragma unroll
  for (int i = 0; i < 20; ++i) row[i] = 0.0;
  {
    double e[3][3][4];                 // entry (a, b) of E as a polynomial: coefficient of x, y, z, 1
#pragma unroll
    for (int ab = 0; ab < 9; ++ab)
#pragma unroll
      for (int c = 0; c < 4; ++c) e[ab / 3][ab % 3][c] = gshfl(nb[c], ab);
    if (g < 9) {
      const int i = g / 3, j = g % 3;
      double tr[10], D[3][10], ei[3][4], ej[3][4];
#pragma unroll
      for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          ei[m][c] = sel3(i, e[0][m][c], e[1][m][c], e[2][m][c]);
          ej[m][c] = sel3(j, e[m][0][c], e[m][1][c], e[m][2][c]);
        }
#pragma unroll
      for (int q = 0; q < 10; ++q) { tr[q] = 0.0; D[0][q] = 0.0; D[1][q] = 0.0; D[2][q] = 0.0; }
#pragma unroll
      for (int ab = 0; ab < 9; ++ab) mul11_acc(tr, e[ab / 3][ab % 3], e[ab / 3][ab % 3], 1.0);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int m = 0; m < 3; ++m) mul11_acc(D[k], ei[m], e[k][m], 1.0);
#pragma unroll
        for (int q = 0; q < 10; ++q) D[k][q] = (k == i) ? D[k][q] - 0.5 * tr[q] : D[k][q];
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) mul21_acc(row, D[k], ej[k]);
    } else {
      double m0[10], m1[10], m2[10];
#pragma unroll
      for (int q = 0; q < 10; ++q) { m0[q] = 0.0; m1[q] = 0.0; m2[q] = 0.0; }
      mul11_acc(m0, e[1][1], e[2][2], 1.0); mul11_acc(m0, e[1][2], e[2][1], -1.0);
      mul11_acc(m1, e[1][2], e[2][0], 1.0); mul11_acc(m1, e[1][0], e[2][2], -1.0);
      mul11_acc(m2, e[1][0], e[2][1], 1.0); mul11_acc(m2, e[1][1], e[2][0], -1.0);
      mul21_acc(row, m0, e[0][0]); mul21_acc(row, m1, e[0][1]); mul21_acc(row, m2, e[0][2]);
    }
  }
  // 3 -- Gauss-Jordan on columns 0..9: the row with the largest entry of column k among the rows not yet used (ties: the
  // lowest lane) becomes row k where it is; pl[k] = its lane
  bool ok = true, used = g >= 10;
  int pl[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    const double mag = fabs(row[k]);
    double best = (used || !(mag >= 0.0)) ? -1.0 : mag;
    int bl = g;
#pragma unroll
    for (int off = kGroup / 2; off > 0; off >>= 1) {
      const double ov = __shfl_xor(best, off, kGroup);
      const int ol = __shfl_xor(bl, off, kGroup);
      if (ov > best || (ov == best && ol < bl)) { best = ov; bl = ol; }
    }
    pl[k] = bl;
    ok = ok && best > 0.0;
    const double piv = gshfl(row[k], bl);
    const double pd = (best > 0.0) ? piv : 1.0;
    const double f = row[k];
#pragma unroll
    for (int c = k; c < 20; ++c) {
      const double pr = gshfl(row[c], bl) / pd;
      row[c] = (g == bl) ? pr : row[c] - f * pr;
    }
    used = used || g == bl;
  }
  // 4 -- B(z) = [ax ay ac], ascending powers of z, from the row pairs (4,5), (6,7), (8,9)
  double ax[3][4], ay[3][4], ac[3][5];
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    double er[10], fr[10];
#pragma unroll
    for (int q = 0; q < 10; ++q) { er[q] = gshfl(row[10 + q], pl[4 + 2 * t]); fr[q] = gshfl(row[10 + q], pl[5 + 2 * t]); }
    ax[t][0] = er[2]; ax[t][1] = er[1] - fr[2]; ax[t][2] = er[0] - fr[1]; ax[t][3] = -fr[0];
    ay[t][0] = er[5]; ay[t][1] = er[4] - fr[5]; ay[t][2] = er[3] - fr[4]; ay[t][3] = -fr[3];
    ac[t][0] = er[9]; ac[t][1] = er[8] - fr[9]; ac[t][2] = er[7] - fr[8]; ac[t][3] = er[6] - fr[7]; ac[t][4] = -fr[6];
  }
  Sturm S;
  {
    double m12[7], m02[7], m01[7], t1[7], t2[7], d0[11], d1[11], d2[11];
    conv<3, 3>(ax[1], ay[2], t1); conv<3, 3>(ax[2], ay[1], t2);
#pragma unroll
    for (int i = 0; i < 7; ++i) m12[i] = t1[i] - t2[i];
    conv<3, 3>(ax[0], ay[2], t1); conv<3, 3>(ax[2], ay[0], t2);
#pragma unroll
    for (int i = 0; i < 7; ++i) m02[i] = t1[i] - t2[i];
    conv<3, 3>(ax[0], ay[1], t1); conv<3, 3>(ax[1], ay[0], t2);
#pragma unroll
    for (int i = 0; i < 7; ++i) m01[i] = t1[i] - t2[i];
    conv<6, 4>(m12, ac[0], d0); conv<6, 4>(m02, ac[1], d1); conv<6, 4>(m01, ac[2], d2);
    double mx = 0.0;
#pragma unroll
    for (int i = 0; i < 11; ++i) { S.c[i] = (d0[i] - d1[i]) + d2[i]; mx = fmax(mx, fabs(S.c[i])); }
#pragma unroll
    for (int i = 0; i < 11; ++i) S.c[i] = S.c[i] / mx;
  }
  // 5 -- the (g+1)-th real root in (-bound, bound]
  sturm_build(S);
  double bound = 0.0;
#pragma unroll
  for (int i = 0; i < 10; ++i) bound = fmax(bound, fabs(S.c[i] / S.c[10]));
  bound = 1.0 + bound;
  const int v_lo = sturm_variations(S, -bound);
  const int total = v_lo - sturm_variations(S, bound);
  double lo = -bound, hi = bound;
  for (int it = 0; it < kSturmSteps; ++it) {
    const double mid = 0.5 * (lo + hi);
    const bool below = v_lo - sturm_variations(S, mid) >= g + 1;     // at least g + 1 roots in (-bound, mid]
    hi = below ? mid : hi;
    lo = below ? lo : mid;
  }
  double z = 0.5 * (lo + hi);
  for (int it = 0; it < kNewtonSteps; ++it) {
    const double f = poly10(S.c, z), df = dpoly10(S.c, z);
    const double cand = z - ((df != 0.0) ? f / df : 0.0);
    z = (fabs(poly10(S.c, cand)) < fabs(f)) ? cand : z;
  }
  bool root_ok = g < total;
  {
    double mag = fabs(S.c[10]);
#pragma unroll
    for (int i = 9; i >= 0; --i) mag = mag * fabs(z) + fabs(S.c[i]);
    root_ok = root_ok && fabs(poly10(S.c, z)) <= kRootResidual * mag;
  }
  // 6 -- [x y 1] ~ the largest of the three cross products of the rows of B(z)
  double bz[3][3];
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    bz[t][0] = ((ax[t][3] * z + ax[t][2]) * z + ax[t][1]) * z + ax[t][0];
    bz[t][1] = ((ay[t][3] * z + ay[t][2]) * z + ay[t][1]) * z + ay[t][0];
    bz[t][2] = (((ac[t][4] * z + ac[t][3]) * z + ac[t][2]) * z + ac[t][1]) * z + ac[t][0];
  }
  double w[3] = {0.0, 0.0, 0.0}, wn = -1.0;
#pragma unroll
  for (int pr = 0; pr < 3; ++pr) {
    const int r0 = (pr == 2) ? 1 : 0, r1 = (pr == 0) ? 1 : 2;           // (0,1), (0,2), (1,2)
    const double c0 = bz[r0][1] * bz[r1][2] - bz[r0][2] * bz[r1][1];
    const double c1 = bz[r0][2] * bz[r1][0] - bz[r0][0] * bz[r1][2];
    const double c2 = bz[r0][0] * bz[r1][1] - bz[r0][1] * bz[r1][0];
    const double n2 = (c0 * c0 + c1 * c1) + c2 * c2;
    if (n2 > wn) { wn = n2; w[0] = c0; w[1] = c1; w[2] = c2; }
  }
  // 7 -- Gauss-Newton on the ten constraints themselves, in the coefficients k of the basis (|k| = 1: the row k^T dk = 0
  // is the eleventh equation).  The degree-10 polynomial loses digits where its roots lie close; the constraints do not.
  double Nb[4][9], k[4] = {w[0], w[1], z * w[2], w[2]};
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int q = 0; q < 9; ++q) Nb[c][q] = gshfl(nb[c], q);
  {
    const double kn = sqrt((k[0] * k[0] + k[1] * k[1]) + (k[2] * k[2] + k[3] * k[3]));
#pragma unroll
    for (int c = 0; c < 4; ++c) k[c] = k[c] / kn;
  }
  double M[9], r[10], r2;
  combine(Nb, k, M);
  r2 = constraint_residual(M, r);
#pragma unroll 1
  for (int it = 0; it < kPolishSteps; ++it) {
    double EtE[9], EEt[9], cof[9], J[4][10];
    mat3_atb(M, M, EtE);
    mat3_abt(M, M, EEt);
    const double tr = (EEt[0] + EEt[4]) + EEt[8];
    cofactors(M, cof);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      double t1[9], t2[9], t3[9], nte[9];
      mat3_ab(Nb[c], EtE, t1);
      mat3_atb(Nb[c], M, nte);
      mat3_ab(M, nte, t2);
      mat3_ab(EEt, Nb[c], t3);
      double ten = M[0] * Nb[c][0], j0 = cof[0] * Nb[c][0];
#pragma unroll
      for (int q = 1; q < 9; ++q) { ten = ten + M[q] * Nb[c][q]; j0 = j0 + cof[q] * Nb[c][q]; }
      J[c][0] = j0;
#pragma unroll
      for (int q = 0; q < 9; ++q) J[c][1 + q] = (2.0 * ((t1[q] + t2[q]) + t3[q]) - 2.0 * ten * M[q]) - tr * Nb[c][q];
    }
    double Hm[4][5];                   // [J^T J + k k^T | -J^T r]
#pragma unroll
    for (int a = 0; a < 4; ++a) {
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        double sum = k[a] * k[b];
#pragma unroll
        for (int q = 0; q < 10; ++q) sum = sum + J[a][q] * J[b][q];
        Hm[a][b] = sum;
      }
      double gsum = 0.0;
#pragma unroll
      for (int q = 0; q < 10; ++q) gsum = gsum + J[a][q] * r[q];
      Hm[a][4] = -gsum;
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {      // elimination without pivoting (symmetric positive definite)
      const double piv = Hm[a][a];
#pragma unroll
      for (int b = a; b < 5; ++b) Hm[a][b] = Hm[a][b] / piv;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i != a) {
          const double f = Hm[i][a];
#pragma unroll
          for (int b = a; b < 5; ++b) Hm[i][b] = Hm[i][b] - f * Hm[a][b];
        }
      }
    }
    double kc[4], Mc[9], rc[10];
#pragma unroll
    for (int c = 0; c < 4; ++c) kc[c] = k[c] + Hm[c][4];
    const double kn = sqrt((kc[0] * kc[0] + kc[1] * kc[1]) + (kc[2] * kc[2] + kc[3] * kc[3]));
#pragma unroll
    for (int c = 0; c < 4; ++c) kc[c] = kc[c] / kn;
    combine(Nb, kc, Mc);
    const double rc2 = constraint_residual(Mc, rc);
    const bool better = rc2 < r2;
    r2 = better ? rc2 : r2;
#pragma unroll
    for (int c = 0; c < 4; ++c) k[c] = better ? kc[c] : k[c];
#pragma unroll
    for (int q = 0; q < 9; ++q) M[q] = better ? Mc[q] : M[q];
#pragma unroll
    for (int q = 0; q < 10; ++q) r[q] = better ? rc[q] : r[q];
  }
  double n2 = M[0] * M[0];
#pragma unroll
  for (int q = 1; q < 9; ++q) n2 = n2 + M[q] * M[q];
  const double nrm = sqrt(n2);
  valid = root_ok && ok && nrm > 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      E[3 * i + j] = M[3 * j + i] / nrm;                                  // X rows pair (p1, p2) as p1^T M p2: transpose
      valid = valid && isfinite(E[3 * i + j]);
    }
}

__device__ __forceinline__ void store_candidate(double* out, uint8_t* vout, const double* E, bool valid) {
#pragma unroll
  for (int q = 0; q < 9; ++q) out[q] = valid ? E[q] : 0.0;
  *vout = valid ? 1 : 0;
}

// [x1 x2, x1 y2, x1, y1 x2, y1 y2, y1, x2, y2, 1] (essential.py:241-243)
__device__ __forceinline__ void epipolar_row(double x1, double y1, double x2, double y2, double* r) {
  r[0] = x1 * x2; r[1] = x1 * y2; r[2] = x1; r[3] = y1 * x2; r[4] = y1 * y2; r[5] = y1; r[6] = x2; r[7] = y2; r[8] = 1.0;
}

// ------------------------------------------------------------------------------------------------ minimal solver
__global__ __launch_bounds__(64) void emat5_kernel(const double* __restrict__ pts1, const double* __restrict__ pts2,
                                                  const int32_t* __restrict__ samples, int B, int N, int H,
                                                  double* __restrict__ outE, uint8_t* __restrict__ out_valid) {
  const int g = threadIdx.x & (kGroup - 1), b = blockIdx.y;
  const long hh = (long)blockIdx.x * (64 / kGroup) + (threadIdx.x / kGroup);
  const bool live = hh < H;
  const int h = live ? (int)hh : H - 1;         // (a group past the end recomputes the last sample and stores nothing)
  const int32_t* smp = samples + (size_t)h * 5;
  const int rg = g < 9 ? g : 0;
  double a[9];
  bool idx_ok = true;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const int id = smp[i];
    idx_ok = idx_ok && id >= 0 && id < N;
    const size_t o = ((size_t)b * N + (idx_ok ? id : 0)) * 2;
    double r[9];
    epipolar_row(pts1[o], pts1[o + 1], pts2[o], pts2[o + 1], r);
    double rr = r[0];
#pragma unroll
    for (int j = 1; j < 9; ++j) rr = (rg == j) ? r[j] : rr;
#pragma unroll
    for (int j = 0; j < 9; ++j) a[j] = (i == 0) ? rr * r[j] : a[j] + rr * r[j];
  }
  double E[9];
  bool valid;
  five_point_from_gram(a, g, E, valid);
  if (live && g < 10) {
    const size_t slot = ((size_t)b * H + h) * 10 + g;
    store_candidate(outE + slot * 9, out_valid + slot, E, valid && idx_ok);
  }
}

// ------------------------------------------------------------------------------------------------ X^T X over many rows
// kInliers: rows = the inliers of hypothesis sel[b][l] of Esrc under thr[b] (grid (L, B)); else rows = all N points of set
// blockIdx.x times their weight (grid (sets, 1))
template <bool kInliers>
__global__ __launch_bounds__(256) void emat_gram_kernel(const double* __restrict__ pts1, const double* __restrict__ pts2,
                                                       const double* __restrict__ weights, const double* __restrict__ Esrc,
                                                       const int32_t* __restrict__ src_counts, const int32_t* __restrict__ sel,
                                                       const double* __restrict__ thr, int N, int Ksrc, int L,
                                                       double* __restrict__ outE, uint8_t* __restrict__ out_valid) {
  __shared__ double red[9][256];
  __shared__ double Ms[9][9];
  __shared__ double cnt_s;
  const int tid = threadIdx.x;
  const size_t set = kInliers ? (size_t)blockIdx.y : (size_t)blockIdx.x;      // which points
  const size_t slot0 = (kInliers ? (size_t)blockIdx.y * L + blockIdx.x : (size_t)blockIdx.x) * 10;
  double Es[9];
  bool src_ok = true;
  double thr_sq = 0.0;
  if (kInliers) {
    src_ok = load_selected(Esrc, src_counts, sel, blockIdx.y, blockIdx.x, Ksrc, L, Es);
    thr_sq = thr[blockIdx.y];
  }
  const double* p1 = pts1 + set * N * 2;
  const double* p2 = pts2 + set * N * 2;
  double acc[45], rows = 0.0;
#pragma unroll
  for (int i = 0; i < 45; ++i) acc[i] = 0.0;
  for (int n = tid; n < N; n += 256) {
    const double x1 = p1[2 * n], y1 = p1[2 * n + 1], x2 = p2[2 * n], y2 = p2[2 * n + 1];
    double m;
    if (kInliers) m = (src_ok && sampson_sq(Es, x1, y1, x2, y2) <= thr_sq) ? 1.0 : 0.0;
    else m = weights ? weights[set * N + n] : 1.0;
    double r[9];
    epipolar_row(x1, y1, x2, y2, r);
    gram_add(acc, r, m);
    rows = rows + ((m != 0.0) ? 1.0 : 0.0);
  }
  const double cnt = gram_reduce(red, acc, Ms, rows);      // (the row count rides in the free slot of the last pass)
  if (tid == 0) cnt_s = cnt;
  __syncthreads();
  if (tid < 64) {            // the four groups of the first wavefront solve the same matrix; the first one stores
    const int g = tid & (kGroup - 1);
    const int rg = g < 9 ? g : 0;
    double a[9], E[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) a[j] = Ms[rg][j];
    bool valid;
    five_point_from_gram(a, g, E, valid);
    if (tid < 10) store_candidate(outE + (slot0 + tid) * 9, out_valid + slot0 + tid, E, valid && cnt_s >= 5.0);
  }
}

}  // namespace vgg

using namespace vgg;

extern "C" {

int vgge_emat_five_point(const double* points1, const double* points2, const int32_t* samples, int num_pairs, int num_points,
                         int num_samples, double* out_emat, uint8_t* out_valid, void* stream) {
  if (num_pairs < 0 || num_points < 5 || num_samples <= 0) return VGG_ERR_INVALID_ARGUMENT;
  if (num_pairs == 0) return VGG_OK;
  if (!points1 || !points2 || !samples || !out_emat || !out_valid) return VGG_ERR_INVALID_ARGUMENT;
  if (num_pairs > 65535) return VGG_ERR_UNSUPPORTED;
  emat5_kernel<<<dim3(div_up(num_samples, 64 / kGroup), num_pairs), 64, 0, (hipStream_t)stream>>>(
      points1, points2, samples, num_pairs, num_points, num_samples, out_emat, out_valid);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vgge_emat_solve(const double* points1, const double* points2, const double* row_weights, long num_sets, int num_points,
                    double* out_emat, uint8_t* out_valid, void* stream) {
  if (num_sets < 0 || num_points < 5) return VGG_ERR_INVALID_ARGUMENT;
  if (num_sets == 0) return VGG_OK;
  if (!points1 || !points2 || !out_emat || !out_valid) return VGG_ERR_INVALID_ARGUMENT;
  if (num_sets > 2147483647L) return VGG_ERR_UNSUPPORTED;
  emat_gram_kernel<false><<<dim3((unsigned)num_sets), 256, 0, (hipStream_t)stream>>>(
      points1, points2, row_weights, nullptr, nullptr, nullptr, nullptr, num_points, 0, 1, out_emat, out_valid);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vgge_emat_score(const double* points1, const double* points2, const double* emat, const uint8_t* emat_valid,
                    const double* max_error_sq, int num_pairs, int num_points, int num_hypotheses, int32_t* out_counts,
                    double* out_residual_sums, void* stream) {
  if (num_pairs < 0 || num_points <= 0 || num_hypotheses <= 0) return VGG_ERR_INVALID_ARGUMENT;
  if (num_pairs == 0) return VGG_OK;
  if (!points1 || !points2 || !emat || !emat_valid || !max_error_sq || !out_counts || !out_residual_sums)
    return VGG_ERR_INVALID_ARGUMENT;
  if (num_pairs > 65535) return VGG_ERR_UNSUPPORTED;
  two_view_score_kernel<kHypPerWave><<<dim3(div_up(num_hypotheses, 4 * kHypPerWave), num_pairs), 256, 0, (hipStream_t)stream>>>(
      points1, points2, nullptr, emat, emat_valid, max_error_sq, 0.0, num_pairs, num_points, num_hypotheses, out_counts,
      out_residual_sums);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vgge_emat_refine(const double* points1, const double* points2, const double* src_emat, const int32_t* src_counts,
                     const int32_t* selected, const double* max_error_sq, int num_pairs, int num_points, int num_src,
                     int num_selected, double* out_emat, uint8_t* out_valid, void* stream) {
  if (num_pairs < 0 || num_points <= 0 || num_src <= 0 || num_selected <= 0) return VGG_ERR_INVALID_ARGUMENT;
  if (num_pairs == 0) return VGG_OK;
  if (!points1 || !points2 || !src_emat || !src_counts || !selected || !max_error_sq || !out_emat || !out_valid)
    return VGG_ERR_INVALID_ARGUMENT;
  if (num_pairs > 65535) return VGG_ERR_UNSUPPORTED;
  emat_gram_kernel<true><<<dim3(num_selected, num_pairs), 256, 0, (hipStream_t)stream>>>(
      points1, points2, nullptr, src_emat, src_counts, selected, max_error_sq, num_points, num_src, num_selected, out_emat,
      out_valid);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

}  // extern "C"
