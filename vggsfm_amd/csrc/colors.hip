// Point colours of the video path, the reference's VideoRunner._update_points_color (vggsfm/runners/video_runner.py:475-492):
// every 3D point gets the float32 mean of the pixels it was tracked at.
// Two entries.  vgg_color_gather runs frame-major over the observations of a chunk of frames (the rows of a frame are
// neighbours, so its pixels are read while the frame is resident) and stores every observation's (r, g, b, contributes)
// once, at its point-major row: the chunking decides nothing but when a row is written.  vgg_color_reduce then sums each
// point's rows in table order (ascending frame) with plain float32 adds and divides by the count, one thread per point:
// a fixed order, so the result is bit-reproducible and independent of the chunking and of where the frames live.
// Compiled with -ffp-contract=off (there is nothing to contract, but the file is a parity file like the others).
#include <climits>

#include "common.hpp"
#include "../../include/vggsfm_amd.h"

namespace vgg {
namespace {

constexpr int kThreads = 256;

// torch.floor(uv).long() of a float32: floor, then the conversion; values outside int64 and NaN become INT64_MIN (what
// the x86 conversion of the reference's CPU run returns), which passes the upper bounds test and then fails as an index
__device__ __forceinline__ long long floor_to_i64(float x) {
  const float f = floorf(x);
  if (!(f >= -9.223372036854775808e18f && f < 9.223372036854775808e18f)) return LLONG_MIN;
  return (long long)f;
}

// Python / torch indexing of a dimension of size n: -n <= i < n, negative i counts from the end; -1 when out of range
__device__ __forceinline__ long long wrap_index(long long i, long long n) {
  if (i < 0) i += n;
  return (i >= 0 && i < n) ? i : -1;
}

// rows row_begin .. row_end-1 of `order` (point-major observation indices grouped by frame); frames holds frames
// frame_begin .. frame_end-1 as (n, 3, H, W) float32
__global__ void __launch_bounds__(kThreads) color_gather_kernel(const float* __restrict__ frames, int frame_begin, int frame_end,
                                                                int H, int W, int reverse, const int64_t* __restrict__ order,
                                                                long row_begin, long row_end, long num_obs,
                                                                const int64_t* __restrict__ obs_frame,
                                                                const float* __restrict__ obs_uv, float4* __restrict__ gathered,
                                                                int32_t* __restrict__ bad_obs) {
  const long row = row_begin + (long)blockIdx.x * kThreads + threadIdx.x;
  if (row >= row_end) return;
  const long long o = order[row];
  if (o < 0 || o >= num_obs) {                           // (a broken order: nothing to write to; reported as row 0)
    atomicMin(bad_obs, 0);
    return;
  }
  const long long f = obs_frame[o];
  const float2 uv = reinterpret_cast<const float2*>(obs_uv)[o];
  const long long u = floor_to_i64(uv.x), v = floor_to_i64(uv.y);
  float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
  if (v < H && u < W) {                                  // the reference's test; no lower bound
    // images[0, f, :, v, u], or images[0, f, :, u, v] with reverse: the first index runs over H, the second over W
    const long long y = wrap_index(reverse ? u : v, H), x = wrap_index(reverse ? v : u, W);
    if (y < 0 || x < 0 || f < frame_begin || f >= frame_end) {
      atomicMin(bad_obs, (int32_t)o);                    // IndexError in the reference (a frame outside the chunk: caller's)
    } else {
      const size_t plane = (size_t)H * W;
      const float* px = frames + (size_t)(f - frame_begin) * 3 * plane + (size_t)y * W + x;
      out = make_float4(px[0], px[plane], px[2 * plane], 1.f);
    }
  }
  gathered[o] = out;
}

// point_ptr[p] = the first point-major row of point p (num_points + 1 entries; obs_point sorted ascending, in [0, P))
__global__ void __launch_bounds__(kThreads) color_ptr_kernel(const int64_t* __restrict__ obs_point, long num_obs,
                                                             long num_points, int64_t* __restrict__ point_ptr) {
  const long o = (long)blockIdx.x * kThreads + threadIdx.x;
  if (o > num_obs) return;
  long long lo = o == 0 ? -1 : obs_point[o - 1];
  long long hi = o == num_obs ? num_points : obs_point[o];
  lo = lo < -1 ? -1 : (lo > num_points ? num_points : lo);
  hi = hi < -1 ? -1 : (hi > num_points ? num_points : hi);
  for (long long p = lo + 1; p <= hi; ++p) point_ptr[p] = o;
}

__global__ void __launch_bounds__(kThreads) color_reduce_kernel(const float4* __restrict__ gathered, long num_obs,
                                                                long num_points, const int64_t* __restrict__ point_ptr,
                                                                float* __restrict__ rgb, uint8_t* __restrict__ has_color) {
  const long p = (long)blockIdx.x * kThreads + threadIdx.x;
  if (p >= num_points) return;
  long long a = point_ptr[p], b = point_ptr[p + 1];
  a = a < 0 ? 0 : (a > num_obs ? num_obs : a);
  b = b < a ? a : (b > num_obs ? num_obs : b);
  float r = 0.f, g = 0.f, bl = 0.f;
  int n = 0;
  for (long long k = a; k < b; ++k) {
    const float4 c = gathered[k];
    if (c.w != 0.f) {
      r += c.x;
      g += c.y;
      bl += c.z;
      ++n;
    }
  }
  if (n > 0) {                                           // torch's CPU mean: the float32 sum divided by the count
    const float d = (float)n;
    r /= d;
    g /= d;
    bl /= d;
  }
  rgb[3 * p + 0] = r;
  rgb[3 * p + 1] = g;
  rgb[3 * p + 2] = bl;
  has_color[p] = n > 0 ? 1 : 0;
}

}  // namespace
}  // namespace vgg

using namespace vgg;

extern "C" {

int vgg_color_gather(const float* frames, int frame_begin, int frame_end, int height, int width, int reverse,
                     const int64_t* order, long row_begin, long row_end, const int64_t* obs_frame, const float* obs_uv,
                     long num_obs, float* gathered, int32_t* bad_obs, void* stream) {
  if (frame_begin < 0 || frame_end < frame_begin || height <= 0 || width <= 0 || row_begin < 0 || row_end < row_begin ||
      num_obs < 0 || row_end > num_obs)
    return VGG_ERR_INVALID_ARGUMENT;
  if (row_end == row_begin) return VGG_OK;
  if (!frames || !order || !obs_frame || !obs_uv || !gathered || !bad_obs) return VGG_ERR_INVALID_ARGUMENT;
  if (num_obs > 0x7fffffffL) return VGG_ERR_UNSUPPORTED;
  const long rows = row_end - row_begin;
  color_gather_kernel<<<div_up(rows, kThreads), kThreads, 0, (hipStream_t)stream>>>(
      frames, frame_begin, frame_end, height, width, reverse ? 1 : 0, order, row_begin, row_end, num_obs, obs_frame, obs_uv,
      reinterpret_cast<float4*>(gathered), bad_obs);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vgg_color_reduce(const int64_t* obs_point, long num_obs, long num_points, const float* gathered, int64_t* point_ptr,
                     float* rgb, uint8_t* has_color, void* stream) {
  if (num_obs < 0 || num_points < 0) return VGG_ERR_INVALID_ARGUMENT;
  if (num_points == 0) return VGG_OK;
  if (!point_ptr || !rgb || !has_color || (num_obs > 0 && (!obs_point || !gathered))) return VGG_ERR_INVALID_ARGUMENT;
  if (num_obs > 0x7fffffffL || num_points > 0x7fffffffL) return VGG_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  color_ptr_kernel<<<div_up(num_obs + 1, kThreads), kThreads, 0, s>>>(obs_point, num_obs, num_points, point_ptr);
  VGG_LAUNCH_CHECK();
  color_reduce_kernel<<<div_up(num_points, kThreads), kThreads, 0, s>>>(reinterpret_cast<const float4*>(gathered), num_obs,
                                                                       num_points, point_ptr, rgb, has_color);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

}  // extern "C"
