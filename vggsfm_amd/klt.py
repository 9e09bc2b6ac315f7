"""A classical tracker for users without learned weights: grey pyramid, Shi-Tomasi detector and pyramidal Lucas-Kanade as
HIP kernels (csrc/klt/klt.hip); no namesake in the reference, whose tracker is a network.

    build_pyramid / detect_features / track_pair      one kernel entry each (the detector: response + local maxima)
    track_features                                    frames + query points -> pred_track, pred_vis, pred_score in the
                                                      shapes and pixel convention of the reference's predict_tracks
    KLTTracker                                        detect + track, and the extra_tracker callback of
                                                      GeometryRunner.triangulate_extra_points

A point (x, y) with integer coordinates is the centre of pixel [y][x].  What is torch here is plumbing: the global maximum
of the response, the ordering of the selected corners, the frame schedule and the visibility rule of track_features."""
import torch

from . import _lib_klt as K
from ._lib_klt import DIVERGED, FLAT, LEFT, NONFINITE, OK, check, require_gpu, stream_ptr  # noqa: F401

_L = K.lib()          # no fallback: importing the tracker without its library is an error


class Pyramid:
    """`data` (n, floats) float32: per frame all levels in one run, level l at offsets[l] with sizes[l] = (H_l, W_l)."""

    def __init__(self, data, height, width, levels):
        self.data, self.height, self.width, self.levels = data, height, width, levels
        self.sizes, self.offsets = [], []
        h, w, off = height, width, 0
        for l in range(levels):
            if l:
                h, w = (h + 1) // 2, (w + 1) // 2
            self.sizes.append((h, w))
            self.offsets.append(off)
            off += h * w
        assert off == data.shape[1]

    def __len__(self):
        return self.data.shape[0]

    def level(self, l):
        """(n, H_l, W_l) view of level l"""
        h, w = self.sizes[l]
        return self.data[:, self.offsets[l]:self.offsets[l] + h * w].view(-1, h, w)


def _frames4(frames):
    if frames.dim() == 5:
        if frames.shape[0] != 1:
            raise ValueError("the tracker takes one sequence: frames (S,C,H,W) or (1,S,C,H,W)")
        frames = frames[0]
    if frames.dim() != 4 or frames.shape[1] not in (1, 3):
        raise ValueError(f"frames must be (S,3,H,W) or (S,1,H,W), got {tuple(frames.shape)}")
    if frames.dtype != torch.float32:
        raise TypeError(f"frames must be float32, got {frames.dtype}")
    return frames.contiguous()


def build_pyramid(frames, levels=3):
    """frames (n,3,H,W) or (n,1,H,W) float32 (a leading batch dimension of 1 is dropped) -> Pyramid of `levels` levels."""
    frames = _frames4(frames)
    require_gpu(frames)
    n, c, h, w = frames.shape
    floats = int(_L.vggk_pyramid_floats(h, w, levels))
    data = torch.empty(n, floats, dtype=torch.float32, device=frames.device)
    check(_L.vggk_pyramid(frames, n, c, h, w, levels, data, stream_ptr()), "vggk_pyramid")
    return Pyramid(data, h, w, levels)


def _as_pyramid(frames_or_pyramid, levels):
    return frames_or_pyramid if isinstance(frames_or_pyramid, Pyramid) else build_pyramid(frames_or_pyramid, levels)


def corner_response(pyr, frame, window=2):
    """(H, W) float64 Shi-Tomasi response of level 0 of one frame."""
    resp = torch.empty(pyr.height, pyr.width, dtype=torch.float64, device=pyr.data.device)
    check(_L.vggk_corner_response(pyr.level(0)[frame], pyr.height, pyr.width, window, resp, stream_ptr()),
          "vggk_corner_response")
    return resp


def select_features(resp, max_num, quality=0.01, nms_radius=4, border=8, mask=None):
    """Strict local maxima of a response map above quality x its maximum, the best `max_num` first (equal responses: lower
    linear index first) -> (M, 2) float64 xy."""
    require_gpu(resp)
    h, w = resp.shape
    if mask is not None:
        mask = (mask.reshape(h, w) != 0).to(torch.uint8).contiguous()
    flags = torch.empty(h, w, dtype=torch.uint8, device=resp.device)
    gmax = resp.amax().reshape(1)
    check(_L.vggk_local_maxima(resp, h, w, nms_radius, border, quality, gmax, mask, flags, stream_ptr()),
          "vggk_local_maxima")
    idx = torch.nonzero(flags.view(-1)).squeeze(1)                      # ascending linear index
    order = torch.sort(resp.view(-1)[idx], descending=True, stable=True).indices[:max_num]
    idx = idx[order]
    return torch.stack([idx % w, idx // w], dim=1).to(torch.float64)


def detect_features(frames_or_pyramid, frame, max_num, quality=0.01, nms_radius=4, window=2, border=8, mask=None):
    """Shi-Tomasi corners of one frame -> (M, 2) float64 xy, M <= max_num, strongest first."""
    if isinstance(frames_or_pyramid, Pyramid):
        pyr = frames_or_pyramid
    else:                                                   # (only the frame asked for is converted)
        pyr, frame = build_pyramid(_frames4(frames_or_pyramid)[frame:frame + 1], 1), 0
    return select_features(corner_response(pyr, frame, window), max_num, quality, nms_radius, border, mask)


def track_pair(pyr, a, b, points, guess=None, radius=7, max_iters=30, epsilon=0.01, min_eig=1e-6, max_disp=50.0):
    """One pyramidal LK step: the windows around `points` (N,2) of frame a are searched in frame b from `guess` (default:
    the points).  Returns the kernel's raw outputs: positions (N,2) float64, status (N,) int32 (OK / FLAT / LEFT / DIVERGED /
    NONFINITE), zncc (N,) float64, iterations (N,) int32."""
    points = points.to(torch.float64).contiguous()
    guess = points if guess is None else guess.to(torch.float64).contiguous()
    require_gpu(pyr.data, points, guess)
    if points.dim() != 2 or points.shape[1] != 2 or guess.shape != points.shape:
        raise ValueError(f"points and guess must be (N,2), got {tuple(points.shape)} and {tuple(guess.shape)}")
    n, dev = points.shape[0], points.device
    pos = torch.empty(n, 2, dtype=torch.float64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    zncc = torch.empty(n, dtype=torch.float64, device=dev)
    iters = torch.empty(n, dtype=torch.int32, device=dev)
    check(_L.vggk_lk_track(pyr.data[a], pyr.data[b], pyr.height, pyr.width, pyr.levels, points, guess, n, radius, max_iters,
                           epsilon, min_eig, max_disp, pos, status, zncc, iters, stream_ptr()), "vggk_lk_track")
    return pos, status, zncc, iters


def _track_range64(pyr, first, last, query_points, query_frame, fb_threshold, zncc_threshold, lk):
    """track_features over the frames [first, last) of a pyramid; query_frame is an index into the pyramid.  -> the kernel's
    float64 positions (S,N,2), visibility (S,N) bool, score (S,N) float64."""
    pts = query_points.to(torch.float64).reshape(-1, 2).contiguous()
    n, s, dev = pts.shape[0], last - first, pts.device
    track = torch.empty(s, n, 2, dtype=torch.float64, device=dev)
    vis = torch.zeros(s, n, dtype=torch.bool, device=dev)
    score = torch.zeros(s, n, dtype=torch.float64, device=dev)
    track[query_frame - first], vis[query_frame - first], score[query_frame - first] = pts, True, 1.0
    for frames in (range(query_frame + 1, last), range(query_frame - 1, first - 1, -1)):
        guess = pts
        for f in frames:
            pos, st, zncc, _ = track_pair(pyr, query_frame, f, pts, guess, **lk)
            back, st_back, _, _ = track_pair(pyr, f, query_frame, pos, pts, **lk)
            seen = (st == OK) & (st_back == OK) & ((back - pts).norm(dim=1) <= fb_threshold) & (zncc >= zncc_threshold)
            track[f - first], vis[f - first], score[f - first] = pos, seen, zncc.clamp(0, 1)
            guess = torch.where(seen[:, None], pos, guess)
    return track, vis, score


def _track_range(*args):
    """_track_range64 in the shapes and float32 of the reference's predict_tracks"""
    return tuple(t[None].float() for t in _track_range64(*args))


def track_features(frames, query_points, query_frame=0, levels=3, fb_threshold=1.0, zncc_threshold=0.5, **lk):
    """frames (S,C,H,W) (or a Pyramid), query_points (N,2) xy in frame `query_frame` -> pred_track (1,S,N,2), pred_vis
    (1,S,N), pred_score (1,S,N), float32.  The template always comes from the query frame (no drift); the frames are
    visited outwards from it in both directions, each search starting from the track's last visible position in the
    neighbouring frame; each result is tracked back to the query frame with the template taken from the frame just
    tracked.  vis = 1 iff both directions are OK, the round trip ends within fb_threshold of the query point and
    zncc >= zncc_threshold; score = clamp(zncc, 0, 1); the query frame has vis = score = 1.  `lk`: track_pair's options."""
    pyr = _as_pyramid(frames, levels)
    return _track_range(pyr, 0, len(pyr), query_points, query_frame, fb_threshold, zncc_threshold, lk)


class KLTTracker:
    """Detector and tracker over one sequence, its pyramid built once.  `detector`: options of detect_features;
    the remaining options are track_features'."""

    def __init__(self, frames, levels=3, detector=None, fb_threshold=1.0, zncc_threshold=0.5, **lk):
        self.pyramid = build_pyramid(frames, levels)
        self.detector = dict(detector or {})
        self.fb_threshold, self.zncc_threshold, self.lk = fb_threshold, zncc_threshold, lk

    def predict_tracks(self, query_frame=0, max_query_pts=2048, query_points=None):
        """-> pred_track (1,S,N,2), pred_vis (1,S,N), pred_score (1,S,N) from the corners of `query_frame`."""
        if query_points is None:
            query_points = detect_features(self.pyramid, query_frame, max_query_pts, **self.detector)
        return _track_range(self.pyramid, 0, len(self.pyramid), query_points, query_frame, self.fb_threshold,
                            self.zncc_threshold, self.lk)

    def extra_tracker(self, frame_idx, neighbor_start, neighbor_end, grid_points):
        """The callback of GeometryRunner.triangulate_extra_points: grid_points (1,G,2) of frame `frame_idx` tracked
        through the frames [neighbor_start, neighbor_end) -> track (1,S',G,2), vis (1,S',G), score (1,S',G)."""
        return _track_range(self.pyramid, neighbor_start, neighbor_end, grid_points, frame_idx, self.fb_threshold,
                            self.zncc_threshold, self.lk)
