"""NumPy restatement of the tracker's kernels (vggsfm_amd/csrc/klt/vggsfm_amd_klt.h states the arithmetic) and makers of
synthetic frames: sums of Gaussian blobs, whose motion is known analytically.

The pyramid is restated in float32 in the kernel's operation order (bit for bit); everything else in float64, vectorised
over tracks and window pixels, with the window sums taken by ``np.sum`` over the row-major window (``reverse=True``: over
the reversed window -- the spread between the two is what a change of summation order alone does)."""
import functools

import numpy as np

OK, FLAT, LEFT, DIVERGED, NONFINITE = range(5)
F = np.float32


# ------------------------------------------------------------------------------------------------------------ scenes
def render_blobs(height, width, centres, amplitude, sigma):
    """(height, width) float32: sum of Gaussian blobs; centres (n,2) xy with integer = pixel centre."""
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    img = np.zeros((height, width))
    for (cx, cy), a, s in zip(centres, amplitude, sigma):
        img += a * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))
    return img.astype(F)


def blob_scene(height, width, count, seed, margin=12.0, min_dist=0.0):
    """centres (count,2), amplitudes 0.3 .. 1, sigmas 1.5 .. 3; with min_dist the centres keep that distance (sparse scene)."""
    rng = np.random.default_rng(seed)
    centres = []
    for _ in range(200 * count):
        c = rng.uniform([margin, margin], [width - 1 - margin, height - 1 - margin])
        if all(np.hypot(*(c - o)) >= min_dist for o in centres):
            centres.append(c)
        if len(centres) == count:
            break
    else:
        raise ValueError("the blobs do not fit at this distance")
    return np.array(centres), rng.uniform(0.3, 1.0, count), rng.uniform(1.5, 3.0, count)


def translation_frames(height, width, count, shifts, seed, min_dist=0.0, channels=3):
    """frames (len(shifts), channels, H, W) float32 of one blob scene translated by shifts (S,2), and the centres (count,2)
    in frame 0.  3 channels: the grey image in R = G = B (the grey conversion's weights sum to 1 up to rounding)."""
    centres, amp, sig = blob_scene(height, width, count, seed, margin=12.0 + np.abs(shifts).max(), min_dist=min_dist)
    frames = np.stack([render_blobs(height, width, centres + s, amp, sig) for s in np.asarray(shifts, np.float64)])
    return np.ascontiguousarray(np.repeat(frames[:, None], channels, axis=1)), centres


# ------------------------------------------------------------------------------------------------------------ pyramid
def grey(frames):
    frames = np.asarray(frames, F)
    if frames.shape[1] == 1:
        return frames[:, 0].copy()
    g = F(0.299) * frames[:, 0] + F(0.587) * frames[:, 1]
    return g + F(0.114) * frames[:, 2]


def _tap5(a):
    s = F(0.0625) * a[0] + F(0.25) * a[1]
    s = s + F(0.375) * a[2]
    s = s + F(0.25) * a[3]
    return s + F(0.0625) * a[4]


def down(level):
    """(n, H, W) float32 -> (n, (H+1)//2, (W+1)//2)"""
    n, H, W = level.shape
    cols = [np.clip(2 * np.arange((W + 1) // 2) + i - 2, 0, W - 1) for i in range(5)]
    h = _tap5([level[:, :, c] for c in cols])                              # (n, H, W') at the kept columns
    rows = [np.clip(2 * np.arange((H + 1) // 2) + j - 2, 0, H - 1) for j in range(5)]
    return _tap5([h[:, r, :] for r in rows])


def pyramid(frames, levels):
    """list of (n, H_l, W_l) float32; ValueError where the kernel refuses the level count"""
    out = [grey(frames)]
    if not 1 <= levels <= 8:
        raise ValueError("levels")
    for _ in range(1, levels):
        if out[-1].shape[1:] == (1, 1):
            raise ValueError("a level cannot be built from a 1 x 1 level")
        out.append(down(out[-1]))
    return out


def flat_pyramid(levels_list):
    """the kernel's layout: (n, floats)"""
    return np.concatenate([l.reshape(l.shape[0], -1) for l in levels_list], axis=1)


# ------------------------------------------------------------------------------------------------------------ detector
def corner_response(img, window):
    """(H, W) float64 response and trace (gxx + gyy) / area (the scale of the comparison's bound)"""
    I = np.asarray(img, np.float64)
    H, W = I.shape
    P = np.pad(I, 1, mode="edge")
    ix, iy = 0.5 * (P[1:-1, 2:] - P[1:-1, :-2]), 0.5 * (P[2:, 1:-1] - P[:-2, 1:-1])
    area = (2 * window + 1) ** 2
    pad = lambda a: np.pad(a, window, mode="edge")
    xx, xy, yy = pad(ix * ix), pad(ix * iy), pad(iy * iy)
    g = [sum(a[dy:dy + H, dx:dx + W] for dy in range(2 * window + 1) for dx in range(2 * window + 1)) for a in (xx, xy, yy)]
    gxx, gxy, gyy = g
    return 0.5 * ((gxx + gyy) - np.sqrt((gxx - gyy) ** 2 + 4 * gxy * gxy)) / area, (gxx + gyy) / area


def select(resp, max_num, quality=0.01, nms_radius=4, border=8, mask=None):
    """the selection of vggsfm_amd.klt.select_features on a response map -> (M,2) float64 xy"""
    H, W = resp.shape
    thr = quality * resp.max()
    found = []
    for y in range(border, H - border):
        for x in range(border, W - border):
            v = resp[y, x]
            if not v > thr or (mask is not None and not mask[y, x]):
                continue
            y0, y1, x0, x1 = max(y - nms_radius, 0), min(y + nms_radius, H - 1), max(x - nms_radius, 0), min(x + nms_radius, W - 1)
            nb = resp[y0:y1 + 1, x0:x1 + 1]
            lin = (np.arange(y0, y1 + 1)[:, None] * W + np.arange(x0, x1 + 1)[None])
            if (nb > v).any() or ((nb == v) & (lin < y * W + x)).any():
                continue
            found.append((y * W + x, v))
    lin = np.array([f[0] for f in found], dtype=np.int64)
    val = np.array([f[1] for f in found])
    lin = lin[np.argsort(-val, kind="stable")][:max_num]
    return np.stack([lin % W, lin // W], axis=1).astype(np.float64).reshape(-1, 2)


# ------------------------------------------------------------------------------------------------------------ LK step
def bilinear(img, x, y):
    H, W = img.shape
    x, y = np.clip(x, 0.0, W - 1.0), np.clip(y, 0.0, H - 1.0)
    xf, yf = np.floor(x), np.floor(y)
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx, fy = x - xf, y - yf
    I = img.astype(np.float64)
    s = ((1.0 - fx) * (1.0 - fy)) * I[y0, x0] + (fx * (1.0 - fy)) * I[y0, x1]
    s = s + ((1.0 - fx) * fy) * I[y1, x0]
    return s + (fx * fy) * I[y1, x1]


def _min_eig(gxx, gxy, gyy):
    return 0.5 * ((gxx + gyy) - np.sqrt((gxx - gyy) ** 2 + 4.0 * (gxy * gxy)))


def _inside(x, y, W, H):
    return (x >= 0.0) & (x <= W - 1.0) & (y >= 0.0) & (y <= H - 1.0)


def lk_track(pyr_a, pyr_b, points, guess=None, radius=7, max_iters=30, epsilon=0.01, min_eig=1e-6, max_disp=50.0,
             reverse=False):
    """One pyramidal LK step; pyr_a, pyr_b: lists of (H_l, W_l) float32 levels.  -> pos (N,2), status (N,), zncc (N,),
    iters (N,), margin (N,): the smallest relative distance of a deciding quantity of the track from its threshold
    (min-eig vs min_eig at every level, |d| vs max_disp, window centres vs the image edge in pixels / the level's size)."""
    points = np.asarray(points, np.float64).reshape(-1, 2)
    guess = points.copy() if guess is None else np.asarray(guess, np.float64).reshape(-1, 2)
    N, side = len(points), 2 * radius + 1
    area = float(side * side)
    oy, ox = [o.reshape(-1).astype(np.float64) for o in np.mgrid[-radius:radius + 1, -radius:radius + 1]]
    if reverse:
        ox, oy = ox[::-1].copy(), oy[::-1].copy()
    tot = lambda a: np.sum(a, axis=-1)
    status = np.zeros(N, np.int32)
    finite = np.isfinite(points).all(1) & np.isfinite(guess).all(1)
    status[~finite] = NONFINITE
    p, g = np.where(finite[:, None], points, 0.0), np.where(finite[:, None], guess, 0.0)
    d = np.zeros((N, 2))
    iters = np.zeros(N, np.int32)
    margin = np.full(N, np.inf)
    T0 = None

    def note(idx, value, threshold, scale=None):
        rel = np.abs(value - threshold) / (np.abs(threshold) if scale is None else scale)
        margin[idx] = np.minimum(margin[idx], rel)

    for l in range(len(pyr_a) - 1, -1, -1):
        A, B = pyr_a[l], pyr_b[l]
        H, W = A.shape
        s = 1.0 / (1 << l)
        pl, q = p * s, g * s
        live = status == OK
        inside = _inside(pl[:, 0], pl[:, 1], W, H)
        edge = np.minimum.reduce([pl[:, 0], W - 1.0 - pl[:, 0], pl[:, 1], H - 1.0 - pl[:, 1]])
        note(live, edge[live], 0.0, float(max(H, W)))
        status[live & ~inside] = LEFT
        live &= inside
        x, y = pl[:, 0:1] + ox[None], pl[:, 1:2] + oy[None]
        T = bilinear(A, x, y)
        Tx = 0.5 * (bilinear(A, x + 1.0, y) - bilinear(A, x - 1.0, y))
        Ty = 0.5 * (bilinear(A, x, y + 1.0) - bilinear(A, x, y - 1.0))
        gxx, gxy, gyy = tot(Tx * Tx), tot(Tx * Ty), tot(Ty * Ty)
        me = _min_eig(gxx, gxy, gyy) / area
        if min_eig > 0:
            note(live, me[live], min_eig)
        flat = ~(me >= min_eig)
        if l == 0:
            status[live & flat] = FLAT
            T0 = T
        run = live & ~flat
        det = gxx * gyy - gxy * gxy
        for _ in range(max_iters):
            if not run.any():
                break
            c = q + d
            inside = _inside(c[:, 0], c[:, 1], W, H)
            edge = np.minimum.reduce([c[:, 0], W - 1.0 - c[:, 0], c[:, 1], H - 1.0 - c[:, 1]])
            note(run, edge[run], 0.0, float(max(H, W)))
            status[run & ~inside] = LEFT
            run &= inside
            e = T - bilinear(B, c[:, 0:1] + ox[None], c[:, 1:2] + oy[None])
            bx, by = tot(e * Tx), tot(e * Ty)
            with np.errstate(all="ignore"):
                sx, sy = (gyy * bx - gxy * by) / det, (gxx * by - gxy * bx) / det
            iters[run] += 1
            bad = run & ~(np.isfinite(sx) & np.isfinite(sy))
            status[bad] = DIVERGED
            run &= ~bad
            d[run, 0] += sx[run]
            d[run, 1] += sy[run]
            step = np.sqrt(sx * sx + sy * sy)
            if epsilon > 0:
                note(run, step[run], epsilon)
            run &= ~(step < epsilon)
        if l > 0:
            d = 2.0 * d
    live = status == OK
    H, W = pyr_a[0].shape
    dist = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2)
    note(live, dist[live], max_disp)
    status[live & ~(dist <= max_disp)] = DIVERGED
    live = status == OK
    c = g + d
    inside = _inside(c[:, 0], c[:, 1], W, H)
    edge = np.minimum.reduce([c[:, 0], W - 1.0 - c[:, 0], c[:, 1], H - 1.0 - c[:, 1]])
    note(live, edge[live], 0.0, float(max(H, W)))
    status[live & ~inside] = LEFT
    ok = status == OK
    Bv = bilinear(pyr_b[0], c[:, 0:1] + ox[None], c[:, 1:2] + oy[None])
    a, b = T0 - (tot(T0) / area)[:, None], Bv - (tot(Bv) / area)[:, None]
    tt, bb, tb = tot(a * a), tot(b * b), tot(a * b)
    den = np.sqrt(tt * bb)
    with np.errstate(all="ignore"):
        zncc = np.where(ok & (den > 0.0), tb / den, 0.0)
    pos = np.where(ok[:, None], guess + d, guess)
    return pos, status, zncc, iters, margin


def track_features(frames, query_points, query_frame=0, levels=3, fb_threshold=1.0, zncc_threshold=0.5, first=0, last=None,
                   **lk):
    """vggsfm_amd.klt.track_features restated -> track (S,N,2) float64, vis (S,N) bool, score (S,N) float64"""
    pyr = pyramid(frames, levels)
    last = len(frames) if last is None else last
    pts = np.asarray(query_points, np.float64).reshape(-1, 2)
    at = lambda f: [lv[f] for lv in pyr]
    S, N = last - first, len(pts)
    track, vis, score = np.zeros((S, N, 2)), np.zeros((S, N), bool), np.zeros((S, N))
    track[query_frame - first], vis[query_frame - first], score[query_frame - first] = pts, True, 1.0
    for order in (range(query_frame + 1, last), range(query_frame - 1, first - 1, -1)):
        guess = pts
        for f in order:
            pos, st, zncc, _, _ = lk_track(at(query_frame), at(f), pts, guess, **lk)
            back, st_back, _, _, _ = lk_track(at(f), at(query_frame), pos, pts, **lk)
            seen = (st == OK) & (st_back == OK) & (np.hypot(*(back - pts).T) <= fb_threshold) & (zncc >= zncc_threshold)
            track[f - first], vis[f - first], score[f - first] = pos, seen, np.clip(zncc, 0, 1)
            guess = np.where(seen[:, None], pos, guess)
    return track, vis, score


# ------------------------------------------------------------------------------------------------------------ shared cases
@functools.lru_cache(maxsize=None)
def translation_case():
    """The pure-translation case of the issue: 96 x 128, 70 blobs, shifts up to 9 px -> (frames (2,3,H,W), centres, shift)"""
    shift = np.array([7.3, -5.2])
    frames, centres = translation_frames(96, 128, 70, np.array([[0.0, 0.0], shift]), seed=5)
    return frames, centres, shift


@functools.lru_cache(maxsize=None)
def sequence_case():
    """6 frames of 96 x 128 under pure translation, 12 px in all -> (frames (6,3,H,W), centres, shifts (6,2))"""
    shifts = np.outer(np.arange(6) / 5.0, np.array([9.6, -7.2]))
    frames, centres = translation_frames(96, 128, 60, shifts, seed=11)
    return frames, centres, shifts


# ------------------------------------------------------------------------------------------------------------ LK cases
def _sparse_pair(height, width, count, shift, seed, margin=12.0, min_dist=22.0):
    centres, amp, sig = blob_scene(height, width, count, seed, margin=margin, min_dist=min_dist)
    frames = np.stack([render_blobs(height, width, centres + s, amp, sig) for s in (np.zeros(2), np.asarray(shift))])
    return np.ascontiguousarray(frames[:, None]), centres


@functools.lru_cache(maxsize=None)
def lk_cases():
    """name -> dict(frames (2,1,H,W), points, guess, levels, kw): the LK cases of tests/test_gpu_klt.py.  At most 40 tracks
    each.  The queries sit off the blob centres by a sub-pixel draw, so that no coordinate is an integer."""
    rng = np.random.default_rng(3)
    frames, centres, shift = translation_case()
    frames = np.ascontiguousarray(frames[:, :1])
    cases = {}
    for n in (1, 3, 4, 5, 37):
        for r in (1, 4, 7):
            for levels in (1, 3):
                pts = centres[:n] + rng.uniform(-0.45, 0.45, (n, 2))
                # the search starts within half a pixel of the truth: inside the basin of every window size and level count
                guess = pts + shift + rng.uniform(-0.4, 0.4, (n, 2))
                cases[f"n{n}_r{r}_l{levels}"] = dict(frames=frames, points=pts, guess=guess, levels=levels, kw=dict(radius=r))
    # the coarsest level (6 x 8) is smaller than the 15 x 15 window
    small, c = _sparse_pair(24, 32, 2, (1.2, -0.8), seed=2, margin=8.0, min_dist=7.0)
    cases["small_24x32"] = dict(frames=small, points=c + rng.uniform(-0.3, 0.3, c.shape), guess=None, levels=3, kw=dict(radius=7))
    # windows that hang over the border: blobs 3 px from the edges
    edge_c = np.array([[3.3, 40.2], [124.1, 50.7], [60.4, 2.6], [70.2, 92.3], [3.8, 3.1]])
    amp, sig = np.linspace(0.5, 1.0, 5), np.linspace(1.6, 2.8, 5)
    sh = np.array([0.8, 0.5])
    edge = np.stack([render_blobs(96, 128, edge_c + s, amp, sig) for s in (np.zeros(2), sh)])[:, None]
    cases["border"] = dict(frames=np.ascontiguousarray(edge), points=edge_c + 0.05, guess=None, levels=3, kw=dict(radius=7))
    # a sparse scene: a query far from every blob is flat; beside it ordinary tracks
    sparse, sc = _sparse_pair(96, 128, 4, (1.5, 1.0), seed=8, margin=20.0, min_dist=30.0)
    yy, xx = np.mgrid[10:86, 10:118]
    far = np.hypot(xx[..., None] - sc[:, 0], yy[..., None] - sc[:, 1]).min(-1)
    fy, fx = np.unravel_index(np.argmax(far), far.shape)
    assert far[fy, fx] > 25
    flat_q = np.array([[xx[fy, fx] + 0.25, yy[fy, fx] + 0.5]])
    cases["flat"] = dict(frames=sparse, points=np.concatenate([sc[:2] + 0.2, flat_q, sc[2:4] - 0.3]), guess=None, levels=3,
                         kw=dict(radius=7), expect={2: FLAT})
    # one level, a guess 40 px off that lands outside the image (left image), and a displacement bound that the true
    # motion exceeds (diverged)
    pts = centres[:5] + 0.3
    guess = pts + shift
    k = int(np.argmax(pts[:, 0]))
    guess[k] = pts[k] + np.array([40.0, 0.0])
    assert guess[k, 0] > 127
    cases["far_guess"] = dict(frames=frames, points=pts, guess=guess, levels=1, kw=dict(radius=7), expect={k: LEFT})
    cases["max_disp"] = dict(frames=frames, points=pts, guess=None, levels=3, kw=dict(radius=7, max_disp=2.0),
                             expect={i: DIVERGED for i in range(5)})
    # non-finite inputs in a workgroup of otherwise ordinary tracks
    pts, guess = centres[:6] + 0.1, centres[:6] + 0.1 + shift
    pts[1, 0], guess[3, 1], guess[4, 0] = np.nan, np.inf, np.nan
    cases["nonfinite"] = dict(frames=frames, points=pts, guess=guess, levels=3, kw=dict(radius=7),
                              expect={1: NONFINITE, 3: NONFINITE, 4: NONFINITE})
    return cases


MODES = {"fixed10": dict(epsilon=0.0, max_iters=10), "eps": dict(epsilon=0.01, max_iters=30)}


@functools.lru_cache(maxsize=None)
def lk_reference(name, mode, reverse=False):
    """(pos, status, zncc, iters, margin) of the restatement for a case of lk_cases() -- computed once, never modified"""
    c = lk_cases()[name]
    pyr = pyramid(c["frames"], c["levels"])
    out = lk_track([l[0] for l in pyr], [l[1] for l in pyr], c["points"], c["guess"], reverse=reverse, **c["kw"], **MODES[mode])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def lk_order_spread():
    """The largest position difference, over all cases of lk_cases() at epsilon = 0 and 10 iterations, between the
    restatement summing each window row-major and reversed.  The GPU tolerance is 100 x this."""
    worst = 0.0
    for name in lk_cases():
        a, b = lk_reference(name, "fixed10"), lk_reference(name, "fixed10", True)
        assert np.array_equal(a[1], b[1]), name
        both = np.isfinite(a[0]) & np.isfinite(b[0])               # (a non-finite guess is returned as it came)
        worst = max(worst, float(np.abs(a[0][both] - b[0][both]).max(initial=0.0)))
    return worst


# ------------------------------------------------------------------------------------------------------------ a 3D scene
SCENE_A = dict(frames=8, height=128, width=160, blobs=120, focal=160.0, arc_deg=6.0, seed=21)
# tracker options of the scene: at this density a 15 x 15 window holds several blobs of different depths, a 9 x 9 one mostly one
SCENE_A_TRACKER = dict(radius=4, detector=dict(nms_radius=2))


def projected_scene(frames=8, height=128, width=160, blobs=120, focal=160.0, arc_deg=6.0, seed=21):
    """Blobs at projected 3D points: vggsfm_amd.scene's camera path (cameras on an arc around the point cloud, looking at its
    centre) with the arc scaled so that neighbouring frames move a blob by 3 px at the most.  -> dict(images (S,3,H,W)
    float32, extrinsics (S,3,4), intrinsics (S,3,3), points3D (n,3), uv (S,n,2), amplitude, sigma)."""
    from vggsfm_amd.scene import make_cameras, project
    ext, K, _ = make_cameras(frames, "SIMPLE_PINHOLE", shared_camera=True, seed=seed, arc_deg=arc_deg, focal=focal)
    K[:, 0, 2], K[:, 1, 2] = width / 2.0, height / 2.0
    rng = np.random.default_rng(seed)
    pts = np.array([0.0, 0.0, 4.0]) + rng.uniform(-1.0, 1.0, (blobs, 3)) * np.array([1.0, 0.75, 1.0])
    amp, sig = rng.uniform(0.3, 1.0, blobs), rng.uniform(1.5, 3.0, blobs)
    uv, _ = project(pts, ext, K, None)
    assert np.abs(np.diff(uv, axis=0)).max() <= 3.0
    grey_frames = np.stack([render_blobs(height, width, uv[s], amp, sig) for s in range(frames)])
    images = np.ascontiguousarray(np.repeat(grey_frames[:, None], 3, axis=1))
    return dict(images=images, extrinsics=ext, intrinsics=K, points3D=pts, uv=uv, amplitude=amp, sigma=sig)


def restated_tracks(images, max_num=2048, radius=7, detector=None):
    """The restatement's detector and tracker (options as KLTTracker's) -> query (N,2), track (S,N,2), vis, score"""
    resp, _ = corner_response(grey(images[:1])[0], 2)
    query = select(resp, max_num, **(detector or {}))
    return (query,) + track_features(images, query, radius=radius)
