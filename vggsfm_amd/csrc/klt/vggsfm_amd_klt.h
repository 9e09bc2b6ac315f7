/*
 * vggsfm_amd -- pyramidal Lucas-Kanade tracker with a Shi-Tomasi detector (libvggsfm_amd_klt.so, a library of its own:
 * the entries of libvggsfm_amd.so and the headers under include/ are a closed, counted set).
 *
 * Conventions of include/vggsfm_amd.h hold: device pointers, `stream` a hipStream_t as void*, asynchronous (no entry
 * synchronises with the host), no allocation, VGG_OK (0) or a negative VGG_ERR_* code.  The names carry the prefix vggk_;
 * their rows stand in vggsfm_amd/_lib_klt.py.
 *
 * Images are float32, row-major; a point (x, y) with integer coordinates is the centre of pixel [y][x].  A pyramid of
 * `levels` levels of an H x W frame is one run of floats: level 0 (H x W) first, level l + 1 of size
 * ((H_l + 1) / 2, (W_l + 1) / 2) behind level l; vggk_pyramid_floats gives its length.  A level may only be built from a
 * level that is larger than 1 x 1: asking for more is VGG_ERR_INVALID_ARGUMENT, and so are levels < 1 or > 8.
 *
 * Pixel arithmetic of the pyramid is float32 in a stated order, everything else float64, all without floating-point
 * contraction.  Every sum is taken in a fixed order and there are no atomics: two runs give the same bits.
 * A count of 0 (frames, tracks) is a no-op that returns VGG_OK.
 */
#ifndef VGGSFM_AMD_KLT_H
#define VGGSFM_AMD_KLT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VGGK_MAX_LEVELS 8
#define VGGK_MAX_RADIUS 7
/* status of a track */
#define VGGK_OK 0
#define VGGK_FLAT 1       /* min-eig(G) / area < min_eig at level 0 */
#define VGGK_LEFT 2       /* a window centre outside [0, W_l - 1] x [0, H_l - 1] */
#define VGGK_DIVERGED 3   /* |d| at level 0 > max_disp, or a step that is not finite */
#define VGGK_NONFINITE 4  /* point or guess not finite */

const char* vggk_build_arch(void);

/* floats of one frame's pyramid; 0 when the sizes or the level count are refused */
size_t vggk_pyramid_floats(int height, int width, int levels);

/* frames (num_frames, channels, height, width), channels 1 or 3 -> pyramid (num_frames, vggk_pyramid_floats).
 * grey = 0.299 R + 0.587 G + 0.114 B, summed left to right (1 channel: copied).  Level l + 1 [y][x] = sum over the taps
 * (1 4 6 4 1) / 16 in tap order of h[2 y + j - 2][2 x], h[r][c] = the same tap sum of level l [r][c + i - 2], rows and
 * columns clamped to the image. */
int vggk_pyramid(const float* frames, int num_frames, int channels, int height, int width, int levels, float* pyramid,
                 void* stream);

/* Shi-Tomasi response of one image: gradients Ix = (I[y][x+1] - I[y][x-1]) / 2, Iy likewise, neighbours clamped; the
 * structure tensor summed over the (2 window + 1)^2 pixels around (x, y), window pixels clamped to the image, row-major;
 * response (height, width) doubles = ((gxx + gyy) - sqrt((gxx - gyy)^2 + 4 gxy^2)) / 2 / area.  window <= 15. */
int vggk_corner_response(const float* image, int height, int width, int window, double* response, void* stream);

/* flags (height, width) uint8: 1 where the response is > quality x *global_max, is at least `border` pixels from every
 * edge, mask (uint8, may be NULL) is not 0 there, and no pixel of the (2 nms_radius + 1)^2 neighbourhood inside the image
 * is larger, nor equal with a lower linear index. */
int vggk_local_maxima(const double* response, int height, int width, int nms_radius, int border, double quality,
                      const double* global_max, const uint8_t* mask, uint8_t* flags, void* stream);

/* One pyramidal LK step for num_tracks tracks: template around points (num_tracks, 2) xy in pyramid_a, searched in
 * pyramid_b (both one frame's pyramid of the sizes given) from guess (num_tracks, 2).  From the coarsest level l to level
 * 0, with s = 2^-l, p = s x point, q = s x guess, d = 0 at the coarsest level and doubled from level to level:
 *   T, Tx, Ty over the (2 radius + 1)^2 window at p (bilinear, coordinates clamped, Tx = (T(x+1) - T(x-1)) / 2),
 *   G = sum [Tx Tx, Tx Ty; Tx Ty, Ty Ty]; a level > 0 with min-eig(G) / area < min_eig is passed over;
 *   at most max_iters times: e = T - B(q + d + offsets), b = sum e (Tx, Ty), step = G^-1 b, d += step, stop once
 *   |step| < epsilon.
 * out_pos (num_tracks, 2) doubles = guess + d, or the guess for a status other than VGGK_OK; out_status int32;
 * out_zncc doubles: zero-mean normalised cross-correlation of T and the final window of B at level 0 (0 when not OK or a
 * window without variance); out_iters int32: steps taken over all levels.  radius 1 .. 7. */
int vggk_lk_track(const float* pyramid_a, const float* pyramid_b, int height, int width, int levels, const double* points,
                  const double* guess, long num_tracks, int radius, int max_iters, double epsilon, double min_eig,
                  double max_disp, double* out_pos, int32_t* out_status, double* out_zncc, int32_t* out_iters, void* stream);

#ifdef __cplusplus
}
#endif
#endif
