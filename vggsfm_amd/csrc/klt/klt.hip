// Pyramidal Lucas-Kanade tracker and Shi-Tomasi detector for gfx950: the entries of vggsfm_amd_klt.h.
// A parity file: built with -ffp-contract=off, every sum in a stated order (tests/klt_cases.py restates it in NumPy).
#include "../common.hpp"
#include "../mvs/mvs_geometry.hpp"
#include "vggsfm_amd_klt.h"

namespace vgg {

constexpr int kMaxLevels = VGGK_MAX_LEVELS;

// one frame's pyramid: offset (floats) and size of every level
struct PyramidLayout {
  long off[kMaxLevels];
  int h[kMaxLevels], w[kMaxLevels];
  int levels;
  long total;
};

// false: sizes or level count refused (vggsfm_amd_klt.h)
static bool pyramid_layout(int H, int W, int levels, PyramidLayout* L) {
  if (H < 1 || W < 1 || levels < 1 || levels > kMaxLevels) return false;
  long off = 0;
  for (int l = 0; l < levels; ++l) {
    if (l > 0) {
      if (H == 1 && W == 1) return false;
      H = (H + 1) / 2;
      W = (W + 1) / 2;
    }
    L->off[l] = off;
    L->h[l] = H;
    L->w[l] = W;
    off += (long)H * W;
  }
  for (int l = levels; l < kMaxLevels; ++l) L->off[l] = 0, L->h[l] = 1, L->w[l] = 1;
  L->levels = levels;
  L->total = off;
  return true;
}

// ------------------------------------------------------------------------------------------------------------ pyramid
__global__ __launch_bounds__(256) void klt_grey_kernel(const float* __restrict__ frames, int channels, long pixels,
                                                      long count, long frame_floats, float* __restrict__ pyr) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const long f = i / pixels, p = i - f * pixels;
  const float* src = frames + f * channels * pixels + p;
  float g;
  if (channels == 3) {
    g = 0.299f * src[0] + 0.587f * src[pixels];
    g = g + 0.114f * src[2 * pixels];
  } else {
    g = src[0];
  }
  pyr[f * frame_floats + p] = g;
}

__device__ __forceinline__ float tap5(float a0, float a1, float a2, float a3, float a4) {
  float s = 0.0625f * a0 + 0.25f * a1;
  s = s + 0.375f * a2;
  s = s + 0.25f * a3;
  s = s + 0.0625f * a4;
  return s;
}

__global__ __launch_bounds__(256) void klt_down_kernel(float* __restrict__ pyr, long frame_floats, long src_off, int Hs,
                                                      int Ws, long dst_off, int Hd, int Wd, long count) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const long per = (long)Hd * Wd;
  const long f = i / per, p = i - f * per;
  const int y = (int)(p / Wd), x = (int)(p - (long)y * Wd);
  const float* src = pyr + f * frame_floats + src_off;
  const int c0 = clampi(2 * x - 2, Ws - 1), c1 = clampi(2 * x - 1, Ws - 1), c2 = clampi(2 * x, Ws - 1),
            c3 = clampi(2 * x + 1, Ws - 1), c4 = clampi(2 * x + 2, Ws - 1);
  float h[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const float* row = src + (long)clampi(2 * y + j - 2, Hs - 1) * Ws;
    h[j] = tap5(row[c0], row[c1], row[c2], row[c3], row[c4]);
  }
  pyr[f * frame_floats + dst_off + p] = tap5(h[0], h[1], h[2], h[3], h[4]);
}

// ------------------------------------------------------------------------------------------------------------ detector
__global__ __launch_bounds__(256) void klt_response_kernel(const float* __restrict__ img, int H, int W, int c,
                                                          double* __restrict__ resp) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)H * W) return;
  const int y = (int)(i / W), x = (int)(i - (long)y * W);
  double gxx = 0.0, gxy = 0.0, gyy = 0.0;
  for (int dy = -c; dy <= c; ++dy) {
    const int yy = clampi(y + dy, H - 1);
    const float* up = img + (long)clampi(yy - 1, H - 1) * W;
    const float* dn = img + (long)clampi(yy + 1, H - 1) * W;
    const float* row = img + (long)yy * W;
    for (int dx = -c; dx <= c; ++dx) {
      const int xx = clampi(x + dx, W - 1);
      const double ix = 0.5 * ((double)row[clampi(xx + 1, W - 1)] - (double)row[clampi(xx - 1, W - 1)]);
      const double iy = 0.5 * ((double)dn[xx] - (double)up[xx]);
      gxx += ix * ix;
      gxy += ix * iy;
      gyy += iy * iy;
    }
  }
  const double area = (double)((2 * c + 1) * (2 * c + 1));
  const double diff = gxx - gyy;
  resp[i] = 0.5 * ((gxx + gyy) - sqrt(diff * diff + 4.0 * (gxy * gxy))) / area;
}

__global__ __launch_bounds__(256) void klt_maxima_kernel(const double* __restrict__ resp, int H, int W, int m, int border,
                                                        double quality, const double* __restrict__ gmax,
                                                        const uint8_t* __restrict__ mask, uint8_t* __restrict__ flags) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)H * W) return;
  const int y = (int)(i / W), x = (int)(i - (long)y * W);
  const double v = resp[i];
  bool keep = v > quality * gmax[0] && x >= border && y >= border && x < W - border && y < H - border;
  if (keep && mask != nullptr) keep = mask[i] != 0;
  if (keep) {
    const int y0 = max(y - m, 0), y1 = min(y + m, H - 1), x0 = max(x - m, 0), x1 = min(x + m, W - 1);
    for (int yy = y0; yy <= y1 && keep; ++yy)
      for (int xx = x0; xx <= x1; ++xx) {
        const long j = (long)yy * W + xx;
        const double u = resp[j];
        if (u > v || (u == v && j < i)) { keep = false; break; }
      }
  }
  flags[i] = keep ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------ LK step
// (clampi and the bilinear sample, coordinates clamped to the image: ../mvs/mvs_geometry.hpp)
__device__ __forceinline__ double min_eig2(double gxx, double gxy, double gyy) {
  const double diff = gxx - gyy;
  return 0.5 * ((gxx + gyy) - sqrt(diff * diff + 4.0 * (gxy * gxy)));
}

struct LkLevels {
  long off[kMaxLevels];
  int h[kMaxLevels], w[kMaxLevels];
};

constexpr int kPerLane = 4;   // (2 * 7 + 1)^2 = 225 window pixels <= 4 * 64

// One wavefront per track, four tracks per workgroup.  Window pixel k = lane + 64 j (j < 4) is row k / side, column
// k % side of the window; T, Tx, Ty of a level stay in registers over its iterations.  Every branch that leaves the level
// or iteration loop is taken on wave_sum results or on the track's own inputs, so the wavefront stays whole.
__global__ __launch_bounds__(256) void klt_lk_kernel(const float* __restrict__ pyr_a, const float* __restrict__ pyr_b,
                                                    LkLevels lv, int levels, const double* __restrict__ points,
                                                    const double* __restrict__ guess, long N, int radius, int max_iters,
                                                    double epsilon, double min_eig, double max_disp,
                                                    double* __restrict__ out_pos, int32_t* __restrict__ out_status,
                                                    double* __restrict__ out_zncc, int32_t* __restrict__ out_iters) {
  const long track = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (track >= N) return;
  const int lane = lane_id();
  const int side = 2 * radius + 1, count = side * side;
  const double area = (double)count;
  const double px = points[2 * track], py = points[2 * track + 1];
  const double gx = guess[2 * track], gy = guess[2 * track + 1];

  double ox[kPerLane], oy[kPerLane];
  bool on[kPerLane];
#pragma unroll
  for (int j = 0; j < kPerLane; ++j) {
    const int k = lane + 64 * j;
    on[j] = k < count;
    const int r = k / side;
    ox[j] = (double)(k - r * side - radius);
    oy[j] = (double)(r - radius);
  }

  int status = VGGK_OK, iters = 0;
  double dx = 0.0, dy = 0.0, zncc = 0.0;
  double T[kPerLane], Tx[kPerLane], Ty[kPerLane];
  if (!(isfinite(px) && isfinite(py) && isfinite(gx) && isfinite(gy))) status = VGGK_NONFINITE;

  for (int l = levels - 1; l >= 0 && status == VGGK_OK; --l) {
    const int H = lv.h[l], W = lv.w[l];
    const float* A = pyr_a + lv.off[l];
    const float* B = pyr_b + lv.off[l];
    const double s = 1.0 / (double)(1 << l);
    const double plx = px * s, ply = py * s, qx = gx * s, qy = gy * s;
    const double xmax = (double)(W - 1), ymax = (double)(H - 1);
    if (!(plx >= 0.0 && plx <= xmax && ply >= 0.0 && ply <= ymax)) { status = VGGK_LEFT; break; }
    double gxx = 0.0, gxy = 0.0, gyy = 0.0;
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
      T[j] = Tx[j] = Ty[j] = 0.0;
      if (on[j]) {
        const double x = plx + ox[j], y = ply + oy[j];
        T[j] = bilinear(A, H, W, x, y);
        Tx[j] = 0.5 * (bilinear(A, H, W, x + 1.0, y) - bilinear(A, H, W, x - 1.0, y));
        Ty[j] = 0.5 * (bilinear(A, H, W, x, y + 1.0) - bilinear(A, H, W, x, y - 1.0));
      }
      gxx += Tx[j] * Tx[j];
      gxy += Tx[j] * Ty[j];
      gyy += Ty[j] * Ty[j];
    }
    gxx = wave_sum(gxx);
    gxy = wave_sum(gxy);
    gyy = wave_sum(gyy);
    const bool flat = !(min_eig2(gxx, gxy, gyy) / area >= min_eig);
    if (flat && l == 0) { status = VGGK_FLAT; break; }
    if (!flat) {
      const double det = gxx * gyy - gxy * gxy;
      for (int it = 0; it < max_iters; ++it) {
        const double cx = qx + dx, cy = qy + dy;
        if (!(cx >= 0.0 && cx <= xmax && cy >= 0.0 && cy <= ymax)) { status = VGGK_LEFT; break; }
        double bx = 0.0, by = 0.0;
#pragma unroll
        for (int j = 0; j < kPerLane; ++j) {
          double e = 0.0;
          if (on[j]) e = T[j] - bilinear(B, H, W, cx + ox[j], cy + oy[j]);
          bx += e * Tx[j];
          by += e * Ty[j];
        }
        bx = wave_sum(bx);
        by = wave_sum(by);
        const double sx = (gyy * bx - gxy * by) / det, sy = (gxx * by - gxy * bx) / det;
        ++iters;
        if (!(isfinite(sx) && isfinite(sy))) { status = VGGK_DIVERGED; break; }
        dx += sx;
        dy += sy;
        if (sqrt(sx * sx + sy * sy) < epsilon) break;
      }
    }
    if (status != VGGK_OK) break;
    if (l > 0) {
      dx = 2.0 * dx;
      dy = 2.0 * dy;
    }
  }

  if (status == VGGK_OK) {
    const int H = lv.h[0], W = lv.w[0];
    const double cx = gx + dx, cy = gy + dy;
    if (!(sqrt(dx * dx + dy * dy) <= max_disp)) {
      status = VGGK_DIVERGED;
    } else if (!(cx >= 0.0 && cx <= (double)(W - 1) && cy >= 0.0 && cy <= (double)(H - 1))) {
      status = VGGK_LEFT;
    } else {
      // T still holds the level-0 template
      double Bv[kPerLane], st = 0.0, sb = 0.0;
#pragma unroll
      for (int j = 0; j < kPerLane; ++j) {
        Bv[j] = 0.0;
        if (on[j]) Bv[j] = bilinear(pyr_b + lv.off[0], H, W, cx + ox[j], cy + oy[j]);
        st += T[j];
        sb += Bv[j];
      }
      const double mt = wave_sum(st) / area, mb = wave_sum(sb) / area;
      double tt = 0.0, bb = 0.0, tb = 0.0;
#pragma unroll
      for (int j = 0; j < kPerLane; ++j) {
        const double a = on[j] ? T[j] - mt : 0.0, b = on[j] ? Bv[j] - mb : 0.0;
        tt += a * a;
        bb += b * b;
        tb += a * b;
      }
      tt = wave_sum(tt);
      bb = wave_sum(bb);
      tb = wave_sum(tb);
      const double den = sqrt(tt * bb);
      zncc = den > 0.0 ? tb / den : 0.0;
    }
  }
  if (lane == 0) {
    const bool ok = status == VGGK_OK;
    out_pos[2 * track] = ok ? gx + dx : gx;
    out_pos[2 * track + 1] = ok ? gy + dy : gy;
    out_status[track] = status;
    out_zncc[track] = ok ? zncc : 0.0;
    out_iters[track] = iters;
  }
}

}  // namespace vgg

using namespace vgg;

extern "C" {

const char* vggk_build_arch(void) { return "gfx950"; }

size_t vggk_pyramid_floats(int height, int width, int levels) {
  PyramidLayout L;
  return pyramid_layout(height, width, levels, &L) ? (size_t)L.total : 0;
}

int vggk_pyramid(const float* frames, int num_frames, int channels, int height, int width, int levels, float* pyramid,
                 void* stream) {
  PyramidLayout L;
  if (num_frames < 0 || (channels != 1 && channels != 3) || !pyramid_layout(height, width, levels, &L))
    return VGG_ERR_INVALID_ARGUMENT;
  if (num_frames == 0) return VGG_OK;
  if (!frames || !pyramid) return VGG_ERR_INVALID_ARGUMENT;
  const long pixels = (long)height * width, count = pixels * num_frames;
  if (count > (long)INT32_MAX * 128) return VGG_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  klt_grey_kernel<<<div_up(count, 256), 256, 0, st>>>(frames, channels, pixels, count, L.total, pyramid);
  VGG_LAUNCH_CHECK();
  for (int l = 1; l < levels; ++l) {
    const long n = (long)L.h[l] * L.w[l] * num_frames;
    klt_down_kernel<<<div_up(n, 256), 256, 0, st>>>(pyramid, L.total, L.off[l - 1], L.h[l - 1], L.w[l - 1], L.off[l],
                                                     L.h[l], L.w[l], n);
    VGG_LAUNCH_CHECK();
  }
  return VGG_OK;
}

int vggk_corner_response(const float* image, int height, int width, int window, double* response, void* stream) {
  if (height < 1 || width < 1 || window < 0 || window > 15 || !image || !response) return VGG_ERR_INVALID_ARGUMENT;
  const long n = (long)height * width;
  if (n > (long)INT32_MAX * 128) return VGG_ERR_UNSUPPORTED;
  klt_response_kernel<<<div_up(n, 256), 256, 0, (hipStream_t)stream>>>(image, height, width, window, response);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vggk_local_maxima(const double* response, int height, int width, int nms_radius, int border, double quality,
                      const double* global_max, const uint8_t* mask, uint8_t* flags, void* stream) {
  if (height < 1 || width < 1 || nms_radius < 0 || border < 0 || !response || !global_max || !flags)
    return VGG_ERR_INVALID_ARGUMENT;
  const long n = (long)height * width;
  if (n > (long)INT32_MAX * 128) return VGG_ERR_UNSUPPORTED;
  klt_maxima_kernel<<<div_up(n, 256), 256, 0, (hipStream_t)stream>>>(response, height, width, nms_radius, border, quality,
                                                                       global_max, mask, flags);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vggk_lk_track(const float* pyramid_a, const float* pyramid_b, int height, int width, int levels, const double* points,
                  const double* guess, long num_tracks, int radius, int max_iters, double epsilon, double min_eig,
                  double max_disp, double* out_pos, int32_t* out_status, double* out_zncc, int32_t* out_iters, void* stream) {
  PyramidLayout L;
  if (num_tracks < 0 || radius < 1 || radius > VGGK_MAX_RADIUS || max_iters < 0 || !pyramid_layout(height, width, levels, &L))
    return VGG_ERR_INVALID_ARGUMENT;
  if (num_tracks == 0) return VGG_OK;
  if (!pyramid_a || !pyramid_b || !points || !guess || !out_pos || !out_status || !out_zncc || !out_iters)
    return VGG_ERR_INVALID_ARGUMENT;
  if (num_tracks > (long)INT32_MAX) return VGG_ERR_UNSUPPORTED;
  LkLevels lv;
  for (int l = 0; l < kMaxLevels; ++l) lv.off[l] = L.off[l], lv.h[l] = L.h[l], lv.w[l] = L.w[l];
  klt_lk_kernel<<<div_up(num_tracks, 4), 256, 0, (hipStream_t)stream>>>(pyramid_a, pyramid_b, lv, levels, points, guess,
                                                                        num_tracks, radius, max_iters, epsilon, min_eig,
                                                                        max_disp, out_pos, out_status, out_zncc, out_iters);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

}  // extern "C"
