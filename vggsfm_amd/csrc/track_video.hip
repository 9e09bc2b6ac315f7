// The track video, the reference's Visualizer.draw_tracks_on_video (vggsfm/utils/visualizer.py:163-295) as the runner calls it
// (runner.py:445-450): per frame, every track's prediction drawn as a small circle over the frame, in track order.
// With integer centres and an integer radius PIL's circle is one of two fixed stencils (filled for a visible point, the
// one-pixel outline otherwise), translated and clipped, and the draws are opaque.  So the painter's order collapses to: a
// pixel takes the colour of the HIGHEST track index whose stencil covers it.  Two entries:
//   vgg_track_owner    one thread per (frame, track): truncates the coordinates as the reference does, applies its skip
//                      and visibility rules and writes track index + 1 with an integer atomicMax into a per-pixel owner
//                      grid through the rows of its stencil.  A maximum does not depend on the order of the atomics, so
//                      the grid, and with it the video, is bit-reproducible.
//   vgg_track_resolve  one pass over the pixels: float frame -> uint8 by truncation, the white border of pad_value, the
//                      owner's colour, the planar output layout and the repetition of frame 0.  A lane takes four
//                      neighbouring pixels of a row and stores one dword per channel.
// Compiled with -ffp-contract=off (the only arithmetic is coordinate + pad, which must round as torch's addition does).
#include "common.hpp"
#include "../../include/vggsfm_amd.h"

namespace vgg {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxRows = 2 * VGG_TRACK_MAX_RADIUS + 1;

struct Stencils {
  uint32_t rows[2][kMaxRows];   // [0]: filled, [1]: outline; row dy + r, bit dx + r
};

// (coordinate + pad).long() of the reference: the addition in the tracks' own precision, then truncation toward zero.
// `ok` is false for a value no frame can be near (NaN, infinite or beyond 2^62): the conversion would not be defined.
template <typename F>
__device__ __forceinline__ long long trunc_coord(F v, int pad, bool& ok) {
  const F s = v + (F)pad;
  ok = ok && (s > (F)-4.611686018427387904e18 && s < (F)4.611686018427387904e18);
  return ok ? (long long)s : 0;
}

// visibility[0, t, i] as the reference's `if visible`: anything but zero (a NaN included; -0.0 is zero)
__device__ __forceinline__ bool is_visible(const void* vis, int kind, size_t k) {
  switch (kind) {
    case VGG_TRACK_VIS_U8: return static_cast<const uint8_t*>(vis)[k] != 0;
    case VGG_TRACK_VIS_F32: return static_cast<const float*>(vis)[k] != 0.f;
    case VGG_TRACK_VIS_F64: return static_cast<const double*>(vis)[k] != 0.0;
    default: return true;
  }
}

// tracks: (T, N, 2) of F; owner: (frame_end - frame_begin, canvas_h, canvas_w), already cleared
template <typename F>
__global__ void __launch_bounds__(kThreads) track_owner_kernel(const F* __restrict__ tracks, const void* __restrict__ vis,
                                                               int vis_kind, int frame_begin, int frame_end, int query_frame,
                                                               long num_tracks, int pad, int canvas_h, int canvas_w, int r,
                                                               Stencils st, uint32_t* __restrict__ owner) {
  // (the highest tracks go first: the later, lower ones then mostly find their pixels taken and skip the atomic)
  const long i = num_tracks - 1 - ((long)blockIdx.x * kThreads + threadIdx.x);
  const int t = frame_begin + (int)blockIdx.y;
  if (i < 0 || t < query_frame || t >= frame_end) return;
  const size_t k = (size_t)t * num_tracks + i;
  bool ok = true;
  const long long x = trunc_coord<F>(tracks[2 * k], pad, ok), y = trunc_coord<F>(tracks[2 * k + 1], pad, ok);
  if (!ok || x == 0 || y == 0) return;                                  // `if coord[0] != 0 and coord[1] != 0`
  if (x + r < 0 || y + r < 0 || x - r >= canvas_w || y - r >= canvas_h) return;   // (64-bit: nothing wraps into the frame)
  const bool filled = is_visible(vis, vis_kind, k);
  const int cx = (int)x, cy = (int)y;
  const uint32_t id = (uint32_t)i + 1u;
  uint32_t* grid = owner + (size_t)(t - frame_begin) * canvas_h * canvas_w;
  for (int dy = -r; dy <= r; ++dy) {
    const int py = cy + dy;
    if (py < 0 || py >= canvas_h) continue;
    uint32_t m = filled ? st.rows[0][dy + r] : st.rows[1][dy + r];     // (a uniform index: both come as scalar loads)
    uint32_t* line = grid + (size_t)py * canvas_w;
    while (m) {
      const int b = __ffs(m) - 1;
      m &= m - 1;
      const int px = cx + b - r;
      // (the plain load only spares atomics: the cell never decreases, so a stale value can only be smaller)
      if (px >= 0 && px < canvas_w && line[px] < id) atomicMax(line + px, id);
    }
  }
}

__device__ __forceinline__ uint32_t to_u8(float v) { return (uint32_t)fminf(fmaxf(v, 0.f), 255.f); }   // NaN -> 0
__device__ __forceinline__ uint32_t to_u8(uint8_t v) { return v; }

// four neighbouring samples of one channel (p 16-byte / 4-byte aligned) as bytes 0..3 of a dword
__device__ __forceinline__ uint32_t load4_u8(const float* p) {
  const float4 v = *reinterpret_cast<const float4*>(p);
  return to_u8(v.x) | to_u8(v.y) << 8 | to_u8(v.z) << 16 | to_u8(v.w) << 24;
}
__device__ __forceinline__ uint32_t load4_u8(const uint8_t* p) { return *reinterpret_cast<const uint32_t*>(p); }

// One lane: pixels x0 .. x0+3 of canvas row y of frame t (frames: the chunk's frames (n, 3, H, W) of P).
// vec_out: canvas_w is a multiple of 4 and out / owner are aligned, so the owners come in as one uint4 and the four pixels
// of a channel go out as one dword.  vec_in: W and pad are multiples of 4 and frames is aligned, so a quad inside the frame
// is one vector load per channel.  Both are uniform over the launch; the scalar paths serve every other shape.
template <typename P>
__global__ void __launch_bounds__(kThreads) track_resolve_kernel(const P* __restrict__ frames, int frame_begin, int frame_end,
                                                                 int H, int W, int pad, const uint32_t* __restrict__ owner,
                                                                 const uint32_t* __restrict__ colors, int color_per_frame,
                                                                 int first_copies, int vec_in, int vec_out,
                                                                 uint8_t* __restrict__ out) {
  const int canvas_h = H + 2 * pad, canvas_w = W + 2 * pad;
  const int quads = (canvas_w + 3) >> 2;
  const long q = (long)blockIdx.x * kThreads + threadIdx.x;
  const long per_frame = (long)quads * canvas_h;
  const int n = frame_end - frame_begin;
  if (q >= per_frame * n) return;
  const int f = (int)(q / per_frame);
  const long rem = q - (long)f * per_frame;
  const int y = (int)(rem / quads), x0 = (int)(rem - (long)y * quads) * 4;
  const int t = frame_begin + f;
  const int sy = y - pad, sx0 = x0 - pad;
  const bool row_in = sy >= 0 && sy < H;
  const size_t plane = (size_t)H * W;
  const P* src = frames + (size_t)f * 3 * plane + (size_t)(row_in ? sy : 0) * W;
  const uint32_t* own = owner + ((size_t)f * canvas_h + y) * canvas_w;
  // the undrawn pixels, four of a channel per dword (byte j = pixel x0 + j): the frame, or the white border of pad_value
  uint32_t ch[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};
  if (row_in && vec_in && sx0 >= 0 && sx0 + 3 < W) {
#pragma unroll
    for (int c = 0; c < 3; ++c) ch[c] = load4_u8(src + c * plane + sx0);
  } else if (row_in) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int sx = sx0 + j;
      if (sx >= 0 && sx < W) {
#pragma unroll
        for (int c = 0; c < 3; ++c) ch[c] = (ch[c] & ~(255u << (8 * j))) | to_u8(src[c * plane + sx]) << (8 * j);
      }
    }
  }
  uint32_t o[4] = {0u, 0u, 0u, 0u};
  if (vec_out) {
    const uint4 v = *reinterpret_cast<const uint4*>(own + x0);
    o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x0 + j < canvas_w) o[j] = own[x0 + j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (o[j]) {                                                        // the highest track drawn here: its colour
      const uint32_t c = colors[color_per_frame ? (uint32_t)t : o[j] - 1u];
      const uint32_t keep = ~(255u << (8 * j));
      ch[0] = (ch[0] & keep) | (c & 255u) << (8 * j);
      ch[1] = (ch[1] & keep) | ((c >> 8) & 255u) << (8 * j);
      ch[2] = (ch[2] & keep) | ((c >> 16) & 255u) << (8 * j);
    }
  }
  // frame 0 stands first_copies times at the head of the output, frame t > 0 at t - 1 + first_copies
  const int copies = t == 0 ? first_copies : 1;
  const int first_out = t == 0 ? 0 : t - 1 + first_copies;
  const size_t cplane = (size_t)canvas_h * canvas_w;
  for (int k = 0; k < copies; ++k) {
    uint8_t* dst = out + (size_t)(first_out + k) * 3 * cplane + (size_t)y * canvas_w + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (vec_out) {
        *reinterpret_cast<uint32_t*>(dst + c * cplane) = ch[c];
      } else {
        for (int j = 0; j < 4 && x0 + j < canvas_w; ++j) dst[c * cplane + j] = (uint8_t)(ch[c] >> (8 * j));
      }
    }
  }
}

}  // namespace
}  // namespace vgg

using namespace vgg;

extern "C" {

int vgg_track_owner(const void* tracks, int tracks_f64, const void* visibility, int vis_kind, int frame_begin, int frame_end,
                    int query_frame, long num_tracks, int pad, int canvas_h, int canvas_w, int radius,
                    const uint32_t* stencil_rows, uint32_t* owner, void* stream) {
  if (frame_begin < 0 || frame_end < frame_begin || num_tracks < 0 || pad < 0 || canvas_h <= 0 || canvas_w <= 0 ||
      radius < 0 || !stencil_rows || vis_kind < VGG_TRACK_VIS_NONE || vis_kind > VGG_TRACK_VIS_F64)
    return VGG_ERR_INVALID_ARGUMENT;
  if (radius > VGG_TRACK_MAX_RADIUS || num_tracks >= 0x7fffffffL || frame_end - frame_begin > 65535)
    return VGG_ERR_UNSUPPORTED;
  const int n = frame_end - frame_begin;
  if (n == 0) return VGG_OK;
  if (!owner || (num_tracks > 0 && (!tracks || (vis_kind != VGG_TRACK_VIS_NONE && !visibility))))
    return VGG_ERR_INVALID_ARGUMENT;
  if ((size_t)n * canvas_h * canvas_w > 0x7fffffffUL) return VGG_ERR_UNSUPPORTED;
  hipStream_t s = (hipStream_t)stream;
  VGG_HIP_CHECK(hipMemsetAsync(owner, 0, (size_t)n * canvas_h * canvas_w * sizeof(uint32_t), s));
  if (num_tracks == 0 || query_frame >= frame_end) return VGG_OK;
  Stencils st;
  memset(&st, 0, sizeof(st));
  const int rows = 2 * radius + 1;
  const uint32_t row_mask = rows == 32 ? 0xffffffffu : ((1u << rows) - 1u);
  for (int k = 0; k < 2; ++k)
    for (int j = 0; j < rows; ++j) st.rows[k][j] = stencil_rows[k * rows + j] & row_mask;   // (never past the bounding box)
  const dim3 grid(div_up(num_tracks, kThreads), n);
  if (tracks_f64)
    track_owner_kernel<double><<<grid, kThreads, 0, s>>>(static_cast<const double*>(tracks), visibility, vis_kind, frame_begin,
                                                         frame_end, query_frame, num_tracks, pad, canvas_h, canvas_w, radius, st,
                                                         owner);
  else
    track_owner_kernel<float><<<grid, kThreads, 0, s>>>(static_cast<const float*>(tracks), visibility, vis_kind, frame_begin,
                                                        frame_end, query_frame, num_tracks, pad, canvas_h, canvas_w, radius, st,
                                                        owner);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

int vgg_track_resolve(const void* frames, int frames_u8, int frame_begin, int frame_end, int height, int width, int pad,
                      const uint32_t* owner, const uint32_t* colors, int color_per_frame, int first_copies, uint8_t* out,
                      void* stream) {
  if (frame_begin < 0 || frame_end < frame_begin || height <= 0 || width <= 0 || pad < 0 || first_copies < 1)
    return VGG_ERR_INVALID_ARGUMENT;
  const int n = frame_end - frame_begin;
  if (n == 0) return VGG_OK;
  if (!frames || !owner || !colors || !out) return VGG_ERR_INVALID_ARGUMENT;
  const long canvas_h = (long)height + 2 * pad, canvas_w = (long)width + 2 * pad;
  if (canvas_w > 0x7ffffff0L || (size_t)n * canvas_h * canvas_w > 0x7fffffffUL) return VGG_ERR_UNSUPPORTED;
  const long quads = (canvas_w + 3) / 4;
  const long lanes = quads * canvas_h * n;
  const int vec_out = canvas_w % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0 &&
                      reinterpret_cast<uintptr_t>(owner) % 16 == 0;
  const int vec_in = width % 4 == 0 && pad % 4 == 0 && reinterpret_cast<uintptr_t>(frames) % 16 == 0;
  hipStream_t s = (hipStream_t)stream;
  if (frames_u8)
    track_resolve_kernel<uint8_t><<<div_up(lanes, kThreads), kThreads, 0, s>>>(
        static_cast<const uint8_t*>(frames), frame_begin, frame_end, height, width, pad, owner, colors, color_per_frame ? 1 : 0,
        first_copies, vec_in, vec_out, out);
  else
    track_resolve_kernel<float><<<div_up(lanes, kThreads), kThreads, 0, s>>>(
        static_cast<const float*>(frames), frame_begin, frame_end, height, width, pad, owner, colors, color_per_frame ? 1 : 0,
        first_copies, vec_in, vec_out, out);
  VGG_LAUNCH_CHECK();
  return VGG_OK;
}

}  // extern "C"
