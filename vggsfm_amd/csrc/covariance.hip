// Covariance of a bundle adjustment on gfx950: include/vggsfm_amd_covariance.h, DESIGN.md section 19.
//
//   vggc_spd_inverse    A^-1 of a symmetric positive-definite matrix: the existing factorisation (vgg_cholesky_solve), then
//                       three kernels of this file -- the 64 x 64 diagonal blocks of L inverted, the block columns of L^-1 as
//                       independent forward substitutions, A^-1 = L^-T L^-1 -- and a copy that mirrors the lower triangle.
//   vggc_ba_covariance  the reduced camera system from the solver's own launches with the damping switched off, inverted, the
//                       Jacobi scaling undone, the blocks cut out; the points' 3 x 3 blocks by a kernel that evaluates the
//                       observations itself.
//
// Matrix-core operand layout (v_mfma_f64_16x16x4_f64, as csrc/chol.hip uses it): with li = lane & 15, lk = lane >> 4 a lane
// passes A[row li][k = lk] and B[k = lk][col li] and receives D[row lk + 4 reg][col li], reg = 0..3.  The rows 4 r .. 4 r + 3 of
// an accumulator tile therefore sit in register r exactly as the B operand of k-step r wants them: a product feeds the
// next one without leaving the registers (trinv_kernel).
// Every sum is taken in a fixed order: per output element the k-steps ascend, and the wave sums are butterflies.
#include "camera_model.hpp"
#include "../../include/vggsfm_amd_covariance.h"

namespace vgg {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kCB = 64;            // block edge of the triangular inverse and of the product
constexpr int kCovMaxN = 46276;    // n + 64 stays below sqrt(2^31): tile counts and block indices fit an int

static inline size_t cov_align(size_t x) { return (x + 255) / 256 * 256; }

// ---------------------------------------------------------------------------------------------
// Row `row` of the lower triangle of A into W (zeros right of the diagonal); row n = the zero right-hand side behind it.
__global__ __launch_bounds__(256) void cov_copy_lower_kernel(const double* __restrict__ A, double* __restrict__ W, int n) {
  const int row = blockIdx.x;
  double* dst = W + (size_t)row * n;
  if (row == n) {
    for (int c = threadIdx.x; c < n; c += 256) dst[c] = 0.0;
    return;
  }
  const double* src = A + (size_t)row * n;
  for (int c = threadIdx.x; c < n; c += 256) dst[c] = (c <= row) ? src[c] : 0.0;
}

// T_b = L_bb^-1 (64 x 64, lower triangular, explicit zeros above the diagonal) for diagonal block b, one wavefront: thread c
// pushes column c of the identity through the forward substitution; rows and columns >= n are padded with the identity.
__global__ __launch_bounds__(64) void cov_diag_inverse_kernel(const double* __restrict__ L, int n, double* __restrict__ T) {
  __shared__ double Ls[kCB * (kCB + 1) / 2];            // the lower triangle, packed by rows (read as broadcasts)
  __shared__ double Xs[kCB][kCB + 1];
  const int b = blockIdx.x, c = threadIdx.x;
  const int r0 = b * kCB;
  for (int r = c; r < kCB; ++r) {
    const int i = r0 + r, j = r0 + c;
    double v = (r == c) ? 1.0 : 0.0;
    if (i < n && j < n) v = L[(size_t)i * n + j];
    Ls[r * (r + 1) / 2 + c] = v;
  }
  __syncthreads();
  for (int r = 0; r < kCB; ++r) {
    double x = 0.0;
    if (r >= c) {
      const double* Lr = Ls + r * (r + 1) / 2;
      double s = (r == c) ? 1.0 : 0.0;
      for (int j = c; j < r; ++j) s -= Lr[j] * Xs[j][c];         // (this thread's own column of Xs)
      x = s / Lr[r];
    }
    Xs[r][c] = x;
  }
  __syncthreads();
  double* dst = T + (size_t)b * kCB * kCB;
  for (int r = 0; r < kCB; ++r) dst[r * kCB + c] = Xs[r][c];
}

// Block column k of M = L^-1, one workgroup; wavefront w owns the 16 columns c0 = 64 k + 16 w .. of it -- every column of
// L^-1 is a forward substitution of its own, so the wavefronts share nothing but the cache:
//   M[k][k] = T_k,   M[i][k] = -T_i sum_{j = k}^{i - 1} L[i][j] M[j][k]   (i > k, 64 x 64 blocks).
// The sum is a 64 x 16 accumulator (four tiles); its registers are the B operands of the product with T_i.  M is written to
// and read back from global memory by the same wavefront (other lanes): the barrier behind every block row orders them (all
// four wavefronts run the same trip count).  Elements of M above the diagonal of block (k, k) are written as the zeros T holds.
__global__ __launch_bounds__(256) void cov_trinv_kernel(const double* __restrict__ L, int n, int nbk, const double* __restrict__ T,
                                                        double* __restrict__ M) {
  const int k = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int li = lane & 15, lk = lane >> 4;
  const int col = k * kCB + 16 * wave + li;             // this lane's column of M (B operand and result)
  const bool col_ok = col < n;
  {
    const double* Tk = T + (size_t)k * kCB * kCB;
    for (int r = lk; r < kCB; r += 4) {
      const int row = k * kCB + r;
      if (row < n && col_ok) M[(size_t)row * n + col] = Tk[r * kCB + 16 * wave + li];
    }
  }
  __syncthreads();
  for (int i = k + 1; i < nbk; ++i) {
    f64x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (f64x4){0.0, 0.0, 0.0, 0.0};
    for (int j = k; j < i; ++j) {
      // the 80 operands of one block product are requested before the first product: the loop is latency bound
      double bv[16], av[4][16];
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int kk = j * kCB + 4 * s + lk;              // (< 64 (nbk - 1) <= n - 1: j <= nbk - 2)
        bv[s] = col_ok ? M[(size_t)kk * n + col] : 0.0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int row = i * kCB + 16 * t + li;
          av[t][s] = (row < n) ? L[(size_t)row * n + kk] : 0.0;
        }
      }
#pragma unroll
      for (int s = 0; s < 16; ++s)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[t][s], bv[s], acc[t], 0, 0, 0);
    }
    const double* Ti = T + (size_t)i * kCB * kCB;
    f64x4 out[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) out[t] = (f64x4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const double bv = acc[s >> 2][s & 3];             // rows 4 s .. 4 s + 3 of the sum: lane (li, lk) holds row 4 s + lk
#pragma unroll
      for (int t = 0; t < 4; ++t)
        out[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(Ti[(16 * t + li) * kCB + 4 * s + lk], bv, out[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = i * kCB + 16 * t + lk + 4 * reg;
        if (row < n && col_ok) M[(size_t)row * n + col] = -out[t][reg];
      }
    __syncthreads();
  }
}

// Lower-triangle tile (I, J), J <= I, of M^T M, one workgroup, a 32 x 32 quadrant per wavefront:
//   out[I][J] = sum_{K >= I} M[K][I]^T M[K][J];  both operands are read along rows of M (coalesced).
__global__ __launch_bounds__(256) void cov_gram_kernel(const double* __restrict__ M, int n, int nbk, double* __restrict__ Out) {
  const int t = blockIdx.x;
  int bi = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
  while ((bi + 1) * (bi + 2) / 2 <= t) ++bi;
  while (bi * (bi + 1) / 2 > t) --bi;
  const int bj = t - bi * (bi + 1) / 2;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int li = lane & 15, lk = lane >> 4;
  const int r0 = bi * kCB + 32 * (wave >> 1), c0 = bj * kCB + 32 * (wave & 1);
  if (c0 > r0 + 31) return;                              // (the quadrant above the diagonal of a diagonal tile)
  f64x4 acc[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int q = 0; q < 2; ++q) acc[m][q] = (f64x4){0.0, 0.0, 0.0, 0.0};
  for (int kb = bi; kb < nbk; ++kb) {
    double a[2][16], b[2][16];                           // (all operands of a 64-deep step requested up front)
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const int kk = kb * kCB + 4 * s + lk;
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const int ca = r0 + 16 * m + li, cb = c0 + 16 * m + li;
        a[m][s] = (kk < n && ca < n) ? M[(size_t)kk * n + ca] : 0.0;
        b[m][s] = (kk < n && cb < n) ? M[(size_t)kk * n + cb] : 0.0;
      }
    }
#pragma unroll
    for (int s = 0; s < 16; ++s)
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[m][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m][s], b[q][s], acc[m][q], 0, 0, 0);
  }
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int i = r0 + 16 * m + lk + 4 * reg, j = c0 + 16 * q + li;
        if (i < n && j < n && j <= i) Out[(size_t)i * n + j] = acc[m][q][reg];
      }
}

// A = the lower triangle of W and its mirror image (32 x 32 tiles through LDS); all NaN when the factorisation failed.
__global__ __launch_bounds__(256) void cov_mirror_kernel(const double* __restrict__ W, int n, double* __restrict__ A,
                                                         const int32_t* __restrict__ fail) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj > bi) return;
  __shared__ double tile[32][33];
  const bool bad = *fail != 0;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    const int i = 32 * bi + r, j = 32 * bj + tx;
    double v = 0.0;
    if (i < n && j < n && j <= i) {
      v = bad ? __builtin_nan("") : W[(size_t)i * n + j];
      A[(size_t)i * n + j] = v;
    }
    tile[r][tx] = v;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int jj = 32 * bj + r, ii = 32 * bi + tx;       // A[jj][ii] = W[ii][jj], strictly above the diagonal
    if (ii < n && jj < n && jj < ii) A[(size_t)jj * n + ii] = tile[tx][r];
  }
}

struct SpdWs {
  double* W;      // n * n + n: the copy that is factored, later the lower triangle of the inverse
  double* T;      // nbk blocks of 64 x 64: L_bb^-1
  void* chol;     // vgg_cholesky_workspace_bytes(n)
  size_t total;
};
static SpdWs spd_carve(int n, void* base) {
  SpdWs w;
  const size_t nbk = (size_t)div_up(n, kCB);
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = cov_align(off + bytes); return (char*)base + o; };
  w.W = (double*)take(8ull * ((size_t)n * n + n));
  w.T = (double*)take(8ull * nbk * kCB * kCB);
  w.chol = (void*)take(vgg_cholesky_workspace_bytes(n));
  w.total = off;
  return w;
}

// ---------------------------------------------------------------------------------------------
// bundle adjustment covariance
struct CovProblem {
  int C, P, NI, model, only_k, shared, loss, n;
  double loss_scale;
  const double *cam_q, *cam_t, *intr, *pts;
  const int32_t *row_ptr, *obs_cam, *col_ptr;
  const float2* obs_uv;
  const uint8_t *cam_const, *intr_const, *pt_const;
};

// which reduced columns take part: what the solver's init_kernel decides for one rank
__global__ void cov_active_kernel(CovProblem pb, int kd, uint8_t* __restrict__ active) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= pb.n) return;
  bool act;
  if (j < 6 * pb.C) {
    const int c = j / 6, k = j - 6 * c;
    const unsigned f = pb.cam_const ? pb.cam_const[c] : 0u;
    act = pb.col_ptr[c + 1] > pb.col_ptr[c];
    if (f & 1u) act = false;
    if (k >= 3 && (f & (2u << (k - 3)))) act = false;
  } else {
    const int a = (j - 6 * pb.C) / kd;
    act = !(pb.intr_const && pb.intr_const[a]);
    if (!pb.shared && !(pb.col_ptr[a + 1] > pb.col_ptr[a])) act = false;
  }
  active[j] = act ? 1 : 0;
}

// the lower triangle of the (Jacobi-scaled) reduced system into `cov`; inactive columns get the unit diagonal and zeros
// (the solver leaves min_lm_diagonal / radius on their diagonal)
__global__ __launch_bounds__(256) void cov_load_kernel(const double* __restrict__ S, const uint8_t* __restrict__ active, int n,
                                                       double* __restrict__ cov) {
  const int row = blockIdx.x;
  const bool ra = active[row] != 0;
  for (int c = threadIdx.x; c <= row; c += 256) {
    double v = S[(size_t)row * n + c];
    if (!ra || !active[c]) v = (c == row) ? 1.0 : 0.0;
    cov[(size_t)row * n + c] = v;
  }
}

// Sigma = D Sigma_scaled D with the solver's Jacobi scales D; zero rows and columns where the column is inactive
__global__ __launch_bounds__(256) void cov_unscale_kernel(const double* __restrict__ scale, const uint8_t* __restrict__ active, int n,
                                                          double* __restrict__ cov) {
  const int row = blockIdx.x;
  const bool ra = active[row] != 0;
  const double sr = scale[row];
  for (int c = threadIdx.x; c < n; c += 256) {
    const double v = cov[(size_t)row * n + c];
    cov[(size_t)row * n + c] = (ra && active[c]) ? (sr * scale[c]) * v : 0.0;
  }
}

// the blocks cut from the reduced covariance
__global__ __launch_bounds__(256) void cov_blocks_kernel(const double* __restrict__ cov, int n, int C, int NI, int kd,
                                                         double* __restrict__ out_pose, double* __restrict__ out_intr,
                                                         double* __restrict__ out_pose_intr) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const long n_pose = 36L * C, n_intr = (long)NI * kd * kd, n_pi = 6L * C * kd;
  if (e < n_pose) {
    if (!out_pose) return;
    const int c = (int)(e / 36), r = (int)(e % 36) / 6, k = (int)(e % 6);
    out_pose[e] = cov[(size_t)(6 * c + r) * n + 6 * c + k];
  } else if (e < n_pose + n_intr) {
    if (!out_intr) return;
    const long f = e - n_pose;
    const int a = (int)(f / (kd * kd)), r = (int)(f % (kd * kd)) / kd, k = (int)(f % kd);
    out_intr[f] = cov[(size_t)(6 * C + kd * a + r) * n + 6 * C + kd * a + k];
  } else if (e < n_pose + n_intr + n_pi) {
    if (!out_pose_intr) return;
    const long f = e - n_pose - n_intr;
    const int c = (int)(f / (6 * kd)), r = (int)(f % (6 * kd)) / kd, k = (int)(f % kd);
    const int a = (NI == 1) ? 0 : c;
    out_pose_intr[f] = cov[(size_t)(6 * c + r) * n + 6 * C + kd * a + k];
  }
}

// One observation: the corrected, constant-masked, unscaled Jacobians F (2 x (6 + KD): pose tangent, refined intrinsics) and
// E (2 x 3) -- the blocks the solver linearises with, evaluated here from the quaternion (csrc/camera_model.hpp).
template <int KD>
__device__ __forceinline__ void cov_eval(const CovProblem& pb, int c, const double* X, float2 uv, double* F, double* E) {
  constexpr int BD = 6 + KD;
  const int a = pb.shared ? 0 : c;
  double r[2], Jp[12], Ji[4];
  obs_eval(pb.model, pb.cam_q + 4 * c, pb.cam_t + 3 * c, pb.intr + 4 * a, X, (double)uv.x, (double)uv.y, r, Jp, Ji, E);
#pragma unroll
  for (int row = 0; row < 2; ++row) {
#pragma unroll
    for (int k = 0; k < 6; ++k) F[row * BD + k] = Jp[row * 6 + k];
    if (KD == 2) { F[row * BD + 6] = Ji[row * 2]; F[row * BD + 7] = Ji[row * 2 + 1]; }
    if (KD == 1) F[row * BD + 6] = pb.only_k ? Ji[row * 2 + 1] : Ji[row * 2];
  }
  if (pb.loss != kLossTrivial) {
    const double s = r[0] * r[0] + r[1] * r[1];
    double rho[3];
    loss_eval(pb.loss, pb.loss_scale, s, rho);
    Corrector cr(s, rho);
    cr.jac<BD>(r, F);
    cr.jac<3>(r, E);
  }
  const unsigned camflag = pb.cam_const ? pb.cam_const[c] : 0u;
  if (camflag) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (camflag & 1u) { F[k] = 0; F[BD + k] = 0; }
      if ((camflag & 1u) || (camflag & (2u << k))) { F[3 + k] = 0; F[BD + 3 + k] = 0; }
    }
  }
  if (KD > 0 && pb.intr_const && pb.intr_const[a]) {
#pragma unroll
    for (int k = 0; k < KD; ++k) { F[6 + k] = 0; F[BD + 6 + k] = 0; }
  }
}

// Sigma_pp = V^-1 + G Sigma_uu G^T, one wavefront per point.  V = sum E^T E is inverted as the solver's point pass inverts its
// block: Cholesky of the Jacobi-scaled block (no damping here), V^-1 = (S L^-T)(S L^-T)^T.  The columns u come in SLOTS: one per
// observation -- the camera's six columns, with per-camera intrinsics its KD intrinsics columns as well -- and, with shared
// intrinsics, one more for those; G_slot = V^-1 E^T F (3 x BW).  The double sum over slot pairs runs in chunks of 64: the
// G of the 64 slots of chunk i go through LDS, every lane keeps the G of its slot j of chunk j in registers and walks the
// slots i in order; a track longer than a wavefront takes several chunks (and re-evaluates an observation once per chunk pair).
template <int KD, bool SHARED>
__global__ __launch_bounds__(256) void cov_points_kernel(CovProblem pb, const double* __restrict__ cov, double* __restrict__ out,
                                                         int32_t* __restrict__ fail) {
  constexpr int BD = 6 + KD;
  constexpr int BW = SHARED ? 6 : BD;                    // columns of a slot
  constexpr int KS = (SHARED && KD > 0) ? KD : 1;
  constexpr bool kSharedSlot = SHARED && KD > 0;
  __shared__ double Gs[4][64][3 * BW + 1];
  __shared__ int32_t B0s[4][64], B1s[4][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = pb.n;
  for (int p = blockIdx.x * 4 + wave; p < pb.P; p += gridDim.x * 4) {
    const int o0 = pb.row_ptr[p], o1 = pb.row_ptr[p + 1];
    const int len = o1 - o0;
    double* dst = out + 9 * (size_t)p;
    if (len <= 0 || (pb.pt_const && pb.pt_const[p])) {
      if (lane < 9) dst[lane] = 0.0;
      continue;
    }
    const double X[3] = {pb.pts[3 * (size_t)p], pb.pts[3 * (size_t)p + 1], pb.pts[3 * (size_t)p + 2]};
    double V[6] = {0, 0, 0, 0, 0, 0}, Wa[3 * KS];
#pragma unroll
    for (int i = 0; i < 3 * KS; ++i) Wa[i] = 0.0;
    for (int o = o0 + lane; o < o1; o += 64) {
      double F[2 * BD], E[6];
      cov_eval<KD>(pb, pb.obs_cam[o], X, pb.obs_uv[o], F, E);
      V[0] += E[0] * E[0] + E[3] * E[3]; V[1] += E[0] * E[1] + E[3] * E[4]; V[2] += E[0] * E[2] + E[3] * E[5];
      V[3] += E[1] * E[1] + E[4] * E[4]; V[4] += E[1] * E[2] + E[4] * E[5]; V[5] += E[2] * E[2] + E[5] * E[5];
      if (kSharedSlot) {
#pragma unroll
        for (int m = 0; m < KS; ++m)
#pragma unroll
          for (int b = 0; b < 3; ++b) Wa[m * 3 + b] += F[6 + m] * E[b] + F[BD + 6 + m] * E[3 + b];
      }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) V[i] = wave_sum(V[i]);
    if (kSharedSlot) {
#pragma unroll
      for (int i = 0; i < 3 * KS; ++i) Wa[i] = wave_sum(Wa[i]);
    }
    // V^-1 through the Cholesky factor of the scaled block
    double s[3];
    s[0] = 1.0 / (1.0 + sqrt(V[0])); s[1] = 1.0 / (1.0 + sqrt(V[3])); s[2] = 1.0 / (1.0 + sqrt(V[5]));
    const double a00 = V[0] * s[0] * s[0], a10 = V[1] * s[0] * s[1], a20 = V[2] * s[0] * s[2];
    const double a11 = V[3] * s[1] * s[1], a21 = V[4] * s[1] * s[2], a22 = V[5] * s[2] * s[2];
    bool ok = a00 > 0;
    const double l00 = sqrt(a00);
    const double l10 = a10 / l00, l20 = a20 / l00;
    const double d11 = a11 - l10 * l10;
    ok = ok && d11 > 0;
    const double l11 = sqrt(d11);
    const double l21 = (a21 - l20 * l10) / l11;
    const double d22 = a22 - l20 * l20 - l21 * l21;
    ok = ok && d22 > 0;
    const double l22 = sqrt(d22);
    if (!ok) {
      if (lane == 0) *fail = 1;
      if (lane < 9) dst[lane] = __builtin_nan("");
      continue;
    }
    const double i00 = 1 / l00, i11 = 1 / l11, i22 = 1 / l22;
    const double i10 = -l10 * i00 * i11;
    const double i21 = -l21 * i11 * i22;
    const double i20 = -(l20 * i00 + l21 * i10) * i22;
    const double g00 = s[0] * i00, g01 = s[0] * i10, g02 = s[0] * i20, g11 = s[1] * i11, g12 = s[1] * i21, g22 = s[2] * i22;
    double Vi[9];
    Vi[0] = g00 * g00 + g01 * g01 + g02 * g02; Vi[1] = g01 * g11 + g02 * g12; Vi[2] = g02 * g22;
    Vi[4] = g11 * g11 + g12 * g12; Vi[5] = g12 * g22; Vi[8] = g22 * g22;
    Vi[3] = Vi[1]; Vi[6] = Vi[2]; Vi[7] = Vi[5];

    const int nslots = len + (kSharedSlot ? 1 : 0);
    // G (3 x BW, row-major) and the column bases of slot `slot` (zeros and column 0 beyond the last slot)
    auto slot_G = [&](const int slot, double* G, int& base0, int& base1) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < 3 * BW; ++i) G[i] = 0.0;
      base0 = 0; base1 = 0;
      if (slot < len) {
        const int o = o0 + slot;
        const int c = pb.obs_cam[o];
        double F[2 * BD], E[6];
        cov_eval<KD>(pb, c, X, pb.obs_uv[o], F, E);
        base0 = 6 * c; base1 = 6 * pb.C + KD * c;
#pragma unroll
        for (int k = 0; k < BW; ++k) {
          const double w0 = E[0] * F[k] + E[3] * F[BD + k], w1 = E[1] * F[k] + E[4] * F[BD + k], w2 = E[2] * F[k] + E[5] * F[BD + k];
#pragma unroll
          for (int a = 0; a < 3; ++a) G[a * BW + k] = Vi[3 * a] * w0 + Vi[3 * a + 1] * w1 + Vi[3 * a + 2] * w2;
        }
      } else if (kSharedSlot && slot == len) {
        base0 = 6 * pb.C;
#pragma unroll
        for (int k = 0; k < KS; ++k)
#pragma unroll
          for (int a = 0; a < 3; ++a) G[a * BW + k] = Vi[3 * a] * Wa[3 * k] + Vi[3 * a + 1] * Wa[3 * k + 1] + Vi[3 * a + 2] * Wa[3 * k + 2];
      }
    };
    // column k of a slot in the reduced system (clamped: the shared slot's unused columns carry G = 0)
    auto column = [&](const int base0, const int base1, const int k) __attribute__((always_inline)) {
      const int c = (SHARED || k < 6) ? base0 + k : base1 + (k - 6);
      return c < n ? c : n - 1;
    };
    double acc[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = 0.0;
    for (int ic = 0; ic < nslots; ic += 64) {
      double Gi[3 * BW];
      int bi0, bi1;
      slot_G(ic + lane, Gi, bi0, bi1);
      __builtin_amdgcn_wave_barrier();                   // (the previous chunk's LDS reads are done: one wavefront, in order)
#pragma unroll
      for (int i = 0; i < 3 * BW; ++i) Gs[wave][lane][i] = Gi[i];
      B0s[wave][lane] = bi0; B1s[wave][lane] = bi1;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int ni = min(64, nslots - ic);
      for (int jc = 0; jc < nslots; jc += 64) {
        double Gj[3 * BW];
        int bj0, bj1;
        if (jc == ic) {
#pragma unroll
          for (int i = 0; i < 3 * BW; ++i) Gj[i] = Gi[i];
          bj0 = bi0; bj1 = bi1;
        } else {
          slot_G(jc + lane, Gj, bj0, bj1);
        }
        if (jc + lane < nslots) {
          for (int i = 0; i < ni; ++i) {
            const double* gi = Gs[wave][i];
            const int b0 = B0s[wave][i], b1 = B1s[wave][i];
#pragma unroll
            for (int kj = 0; kj < BW; ++kj) {
              const int cj = column(bj0, bj1, kj);
              double t0 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
              for (int ki = 0; ki < BW; ++ki) {
                const double sv = cov[(size_t)column(b0, b1, ki) * n + cj];
                t0 += gi[ki] * sv; t1 += gi[BW + ki] * sv; t2 += gi[2 * BW + ki] * sv;
              }
#pragma unroll
              for (int b = 0; b < 3; ++b) {
                acc[b] += t0 * Gj[b * BW + kj]; acc[3 + b] += t1 * Gj[b * BW + kj]; acc[6 + b] += t2 * Gj[b * BW + kj];
              }
            }
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] = wave_sum(acc[i]);
    if (lane == 0) {
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) {
          const double v = Vi[3 * a + b] + 0.5 * (acc[3 * a + b] + acc[3 * b + a]);
          dst[3 * a + b] = v; dst[3 * b + a] = v;
        }
    }
  }
}

struct BaCovWs {
  void* ba;            // the solver's workspace (vgg_ba_workspace_bytes)
  size_t ba_bytes;
  double* cov;         // n * n
  uint8_t* active;     // n
  void* spd;           // vggc_spd_inverse_workspace_bytes(n)
  size_t total;
};

static vgg_ba_options cov_options(const vgg_ba_options* options) {
  vgg_ba_options o = *options;
  // 2^900: the damping clip(colsq s^2, min_lm_diagonal, max_lm_diagonal) / radius of an active column is at most 2^-900 of
  // its scaled diagonal element when that is >= min_lm_diagonal, and min_lm_diagonal 2^-900 (no underflow for any
  // min_lm_diagonal >= 1e-36) beside an element of at least ~1e-250 otherwise: gone in the addition either way
  o.initial_trust_region_radius = ldexp(1.0, 900);
  o.overlap_factorization = 0;      // (the overlap mode leaves the later tile batches to phase 2)
  return o;
}

static int cov_dims(const vgg_ba_problem* pb, int* kd, int* n) {
  if (pb->num_cams < 0 || pb->num_pts < 0 || pb->num_obs < 0) return VGG_ERR_INVALID_ARGUMENT;
  if (pb->num_cams > 0 && pb->num_intr != 1 && pb->num_intr != pb->num_cams) return VGG_ERR_UNSUPPORTED;
  if (pb->camera_model != kPinhole && pb->camera_model != kSimpleRadial) return VGG_ERR_UNSUPPORTED;
  *kd = (pb->refine_focal ? 1 : 0) + ((pb->refine_extra && pb->camera_model == kSimpleRadial) ? 1 : 0);
  const long nn = 6L * pb->num_cams + (long)*kd * pb->num_intr;
  if (nn > kCovMaxN) return VGG_ERR_UNSUPPORTED;
  *n = (int)nn;
  return VGG_OK;
}

static BaCovWs ba_cov_carve(const vgg_ba_problem* pb, const vgg_ba_options* opt2, int n, void* base) {
  BaCovWs w;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = cov_align(off + bytes); return (char*)base + o; };
  w.ba_bytes = vgg_ba_workspace_bytes(pb, opt2);
  w.ba = (void*)take(w.ba_bytes);
  w.cov = (double*)take(8ull * (size_t)n * n);
  w.active = (uint8_t*)take((size_t)n);
  w.spd = (void*)take(spd_carve(n, nullptr).total);
  w.total = off;
  return w;
}

}  // namespace vgg

using namespace vgg;

extern "C" {

size_t vggc_spd_inverse_workspace_bytes(int n) {
  if (n <= 0 || n > kCovMaxN) return 0;
  return spd_carve(n, nullptr).total;
}

int vggc_spd_inverse(double* A, int n, void* workspace, int32_t* device_fail, void* stream) {
  if (n < 0) return VGG_ERR_INVALID_ARGUMENT;
  if (n == 0) return VGG_OK;
  if (!A || !workspace || !device_fail) return VGG_ERR_INVALID_ARGUMENT;
  if (n > kCovMaxN) return VGG_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const SpdWs w = spd_carve(n, workspace);
  const int nbk = div_up(n, kCB);
  cov_copy_lower_kernel<<<n + 1, 256, 0, st>>>(A, w.W, n);
  VGG_LAUNCH_CHECK();
  const int rc = vgg_cholesky_solve(w.W, w.W + (size_t)n * n, n, w.chol, device_fail, stream);
  if (rc != VGG_OK) return rc;
  cov_diag_inverse_kernel<<<nbk, 64, 0, st>>>(w.W, n, w.T);
  VGG_LAUNCH_CHECK();
  cov_trinv_kernel<<<nbk, 256, 0, st>>>(w.W, n, nbk, w.T, A);            // (A holds L^-1 for the moment)
  VGG_LAUNCH_CHECK();
  cov_gram_kernel<<<nbk * (nbk + 1) / 2, 256, 0, st>>>(A, n, nbk, w.W);
  VGG_LAUNCH_CHECK();
  const int nb32 = div_up(n, 32);
  cov_mirror_kernel<<<dim3(nb32, nb32), 256, 0, st>>>(w.W, n, A, device_fail);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

size_t vggc_ba_covariance_workspace_bytes(const vgg_ba_problem* problem, const vgg_ba_options* options, int flags) {
  (void)flags;
  if (!problem || !options) return 0;
  int kd = 0, n = 0;
  if (cov_dims(problem, &kd, &n) != VGG_OK || n <= 0) return 0;
  const vgg_ba_options o = cov_options(options);
  return ba_cov_carve(problem, &o, n, nullptr).total;
}

int vggc_ba_covariance(const vgg_ba_problem* problem, const vgg_ba_options* options, void* workspace, size_t workspace_bytes,
                       int flags, double* out_reduced, double* out_pose, double* out_intr, double* out_pose_intr,
                       double* out_points, int32_t* device_fail, void* stream) {
  if (!problem || !options) return VGG_ERR_INVALID_ARGUMENT;
  if (flags <= 0 || (flags & ~(VGGC_COV_CAMERAS | VGGC_COV_POINTS))) return VGG_ERR_INVALID_ARGUMENT;
  int kd = 0, n = 0;
  int rc = cov_dims(problem, &kd, &n);
  if (rc != VGG_OK) return rc;
  if (problem->num_cams == 0) return VGG_OK;
  if (!workspace || !device_fail) return VGG_ERR_INVALID_ARGUMENT;
  if ((flags & VGGC_COV_POINTS) && problem->num_pts > 0 && !out_points) return VGG_ERR_INVALID_ARGUMENT;
  if (!problem->cam_q || !problem->cam_t || !problem->intr || !problem->row_ptr || !problem->col_ptr) return VGG_ERR_INVALID_ARGUMENT;
  if (problem->num_pts > 0 && !problem->pts) return VGG_ERR_INVALID_ARGUMENT;
  if (problem->num_obs > 0 && (!problem->obs_cam || !problem->obs_uv)) return VGG_ERR_INVALID_ARGUMENT;
  const vgg_ba_options o = cov_options(options);
  const BaCovWs w = ba_cov_carve(problem, &o, n, workspace);
  if (workspace_bytes < w.total) return VGG_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;

  // the reduced system at the current state: the solver's own launches, no damping
  rc = vgg_ba_begin(problem, &o, w.ba, w.ba_bytes, 0, 1, stream);
  if (rc != VGG_OK) return rc;
  rc = vgg_ba_phase(problem, &o, w.ba, 1, stream);
  if (rc != VGG_OK) return rc;
  double *S = nullptr, *scale = nullptr;
  size_t count = 0;
  rc = vgg_ba_reduce_buffer(problem, &o, w.ba, 1, &S, &count);
  if (rc != VGG_OK) return rc;
  rc = vgg_ba_reduce_buffer(problem, &o, w.ba, 8, &scale, &count);
  if (rc != VGG_OK) return rc;

  CovProblem cp;
  cp.C = problem->num_cams; cp.P = problem->num_pts; cp.NI = problem->num_intr; cp.model = problem->camera_model;
  cp.only_k = (!problem->refine_focal && kd == 1) ? 1 : 0;
  cp.shared = problem->num_intr == 1 ? 1 : 0;
  cp.loss = problem->loss; cp.loss_scale = problem->loss_scale; cp.n = n;
  cp.cam_q = problem->cam_q; cp.cam_t = problem->cam_t; cp.intr = problem->intr; cp.pts = problem->pts;
  cp.row_ptr = problem->row_ptr; cp.obs_cam = problem->obs_cam; cp.col_ptr = problem->col_ptr;
  cp.obs_uv = (const float2*)problem->obs_uv;
  cp.cam_const = problem->cam_const; cp.intr_const = problem->intr_const; cp.pt_const = problem->pt_const;

  cov_active_kernel<<<div_up(n, 256), 256, 0, st>>>(cp, kd > 0 ? kd : 1, w.active);
  VGG_LAUNCH_CHECK();
  cov_load_kernel<<<n, 256, 0, st>>>(S, w.active, n, w.cov);
  VGG_LAUNCH_CHECK();
  rc = vggc_spd_inverse(w.cov, n, w.spd, device_fail, stream);
  if (rc != VGG_OK) return rc;
  cov_unscale_kernel<<<n, 256, 0, st>>>(scale, w.active, n, w.cov);
  VGG_LAUNCH_CHECK();

  if (flags & VGGC_COV_CAMERAS) {
    if (out_reduced) VGG_HIP_CHECK(hipMemcpyAsync(out_reduced, w.cov, 8ull * (size_t)n * n, hipMemcpyDeviceToDevice, st));
    if (out_pose || out_intr || out_pose_intr) {
      const long total = 36L * cp.C + (long)cp.NI * kd * kd + 6L * cp.C * kd;
      cov_blocks_kernel<<<div_up(total, 256), 256, 0, st>>>(w.cov, n, cp.C, cp.NI, kd, out_pose, kd ? out_intr : nullptr,
                                                            kd ? out_pose_intr : nullptr);
      VGG_LAUNCH_CHECK();
    }
  }
  if ((flags & VGGC_COV_POINTS) && cp.P > 0) {
    const int wgs = min(div_up(cp.P, 4), 4096);
    if (cp.shared) {
      if (kd == 0) cov_points_kernel<0, true><<<wgs, 256, 0, st>>>(cp, w.cov, out_points, device_fail);
      else if (kd == 1) cov_points_kernel<1, true><<<wgs, 256, 0, st>>>(cp, w.cov, out_points, device_fail);
      else cov_points_kernel<2, true><<<wgs, 256, 0, st>>>(cp, w.cov, out_points, device_fail);
    } else {
      if (kd == 0) cov_points_kernel<0, false><<<wgs, 256, 0, st>>>(cp, w.cov, out_points, device_fail);
      else if (kd == 1) cov_points_kernel<1, false><<<wgs, 256, 0, st>>>(cp, w.cov, out_points, device_fail);
      else cov_points_kernel<2, false><<<wgs, 256, 0, st>>>(cp, w.cov, out_points, device_fail);
    }
    VGG_LAUNCH_CHECK();
  }
  return VGG_OK;
}

}  // extern "C"
