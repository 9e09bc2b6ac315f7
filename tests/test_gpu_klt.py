"""The tracker's kernels (vggsfm_amd/klt.py, csrc/klt/klt.hip) against the NumPy restatement of tests/klt_cases.py.

Position tolerance at epsilon = 0 and 10 iterations per level: 100 x the spread between two runs of the restatement that
differ only in the order of the window sums (klt_cases.lk_order_spread: 1.4e-14 px over the cases here, so 1.4e-12 px);
the factor covers the butterfly order of the kernel's wave sums, which neither run reproduces.  At epsilon = 0.01 the
positions agree within 2 epsilon: either side may stop one step early, each within epsilon of the same fixed point."""
import numpy as np
import pytest
import torch

from tests import klt_cases as C
from vggsfm_amd import klt

pytestmark = pytest.mark.gpu


def D(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ------------------------------------------------------------------------------------------------------------ pyramid
@pytest.mark.parametrize("size", [(1, 9), (2, 2), (5, 7), (33, 47), (96, 128)])
def test_pyramid_bit_exact(size):
    h, w = size
    rng = np.random.default_rng(h * 131 + w)
    for channels in (3, 1):
        for n in (1, 3):
            frames = rng.uniform(0, 1, (n, channels, h, w)).astype(np.float32)
            for levels in (1, 3, 5):
                try:
                    want = C.flat_pyramid(C.pyramid(frames, levels))
                except ValueError:
                    with pytest.raises(RuntimeError, match="invalid argument"):
                        klt.build_pyramid(D(frames), levels)
                    continue
                pyr = klt.build_pyramid(D(frames), levels)
                got = pyr.data.cpu().numpy()
                assert got.shape == want.shape and got.tobytes() == want.tobytes(), (channels, n, levels)
                assert pyr.sizes[-1] == C.pyramid(frames, levels)[-1].shape[1:]


# ------------------------------------------------------------------------------------------------------------ detector
@pytest.mark.parametrize("size,window", [((12, 16), 7), ((96, 128), 2), ((96, 128), 7)])
def test_corner_response(size, window):
    """|delta| <= 1e-12 x (gxx + gyy) / area: sums of at most 225 float64 products taken in two orders."""
    if size == (12, 16):
        img = np.random.default_rng(1).uniform(0, 1, size).astype(np.float32)      # the window overlaps the border everywhere
    else:
        img = C.pyramid(C.translation_case()[0][:1], 1)[0][0]
    got = klt.corner_response(klt.build_pyramid(D(img[None, None]), 1), 0, window).cpu().numpy()
    want, trace = C.corner_response(img, window)
    excess = np.abs(got - want) - 1e-12 * trace
    print(f"\nmax |delta| {np.abs(got - want).max():.3e}, trace up to {trace.max():.3e}")
    assert got.shape == want.shape and np.isfinite(got).all() and excess.max() <= 0.0


def _plateau_image():
    img = np.zeros((40, 48), np.float32)
    img[18:21, 22:25] = 1.0                                   # a constant 3 x 3 bright square
    return img


def test_selection_on_a_plateau_of_the_response():
    """A constant 3 x 3 square of the response map yields one pixel, the one with the lowest linear index; of two equal
    isolated maxima the one with the lower index comes first."""
    resp = np.zeros((40, 48))
    resp[18:21, 22:25] = 2.0
    resp[30, 10] = resp[12, 36] = 3.0
    got = klt.select_features(D(resp), 10, nms_radius=4, border=8).cpu().numpy()
    assert got.tolist() == [[36.0, 12.0], [10.0, 30.0], [22.0, 18.0]]
    assert np.array_equal(got, C.select(resp, 10, nms_radius=4, border=8))


@pytest.mark.parametrize("case", ["plateau_image", "blobs_all", "blobs_top7", "blobs_mask", "blobs_border"])
def test_selection_matches_restatement_on_the_kernels_response(case):
    """The restatement's selection applied to the kernel's own response map: the same points in the same order."""
    kw = dict(quality=0.01, nms_radius=4, border=8)
    mask = None
    if case == "plateau_image":
        img, max_num = _plateau_image(), 50
    else:
        img = C.pyramid(C.translation_case()[0][:1], 1)[0][0]
        max_num = 7 if case == "blobs_top7" else 500
        if case == "blobs_mask":
            mask = np.zeros(img.shape, bool)
            mask[:, :70] = True
        if case == "blobs_border":
            kw.update(border=20, nms_radius=2, quality=0.2)
    resp = klt.corner_response(klt.build_pyramid(D(img[None, None]), 1), 0, 2)
    got = klt.select_features(resp, max_num, mask=None if mask is None else D(mask), **kw).cpu().numpy()
    want = C.select(resp.cpu().numpy(), max_num, mask=mask, **kw)
    print(f"\n{len(want)} points")
    assert len(want) > 0 and got.shape == want.shape and np.array_equal(got, want)
    if case == "blobs_top7":
        assert len(got) == 7
    if case == "blobs_mask":
        assert got[:, 0].max() < 70
    if case == "blobs_all":
        via = klt.detect_features(D(img[None, None]), 0, max_num, window=2, **kw).cpu().numpy()
        assert np.array_equal(via, got) and 30 <= len(got) < max_num


# ------------------------------------------------------------------------------------------------------------ LK step
def _run(name, mode):
    c = C.lk_cases()[name]
    pyr = klt.build_pyramid(D(c["frames"]), c["levels"])
    guess = None if c["guess"] is None else D(c["guess"])
    return [t.cpu().numpy() for t in klt.track_pair(pyr, 0, 1, D(c["points"]), guess, **c["kw"], **C.MODES[mode])]


def test_no_case_sits_on_a_threshold():
    """The inputs are chosen so that the restatement reports no deciding quantity within 1e-9 relative of its threshold
    (computed on the CPU): statuses are then compared without exception."""
    for name in C.lk_cases():
        for mode in C.MODES:
            assert C.lk_reference(name, mode)[4].min() > 1e-9, (name, mode)
    assert 0 < C.lk_order_spread() < 1e-12


@pytest.mark.parametrize("mode", list(C.MODES))
@pytest.mark.parametrize("name", list(C.lk_cases()))
def test_lk_matches_restatement(name, mode):
    pos, status, zncc, iters = _run(name, mode)
    rpos, rstatus, rzncc, riters, _ = C.lk_reference(name, mode)
    c = C.lk_cases()[name]
    for k, want in c.get("expect", {}).items():
        assert rstatus[k] == want, (k, rstatus[k])
    assert np.array_equal(status, rstatus), (status, rstatus)
    guess = c["points"] if c["guess"] is None else c["guess"]
    bad = rstatus != C.OK
    assert pos[bad].tobytes() == np.asarray(guess, np.float64)[bad].tobytes()          # the guess, bit for bit
    assert (zncc[bad] == 0).all() and np.isfinite(pos[np.isfinite(guess).all(1)]).all() and np.isfinite(zncc).all()
    ok = ~bad
    delta = np.abs(pos[ok] - rpos[ok]).max(initial=0.0)
    tol = 100 * C.lk_order_spread() if mode == "fixed10" else 2 * C.MODES[mode]["epsilon"]
    print(f"\nmax |delta pos| {delta:.3e} (tolerance {tol:.3e}), max |delta zncc| {np.abs(zncc - rzncc).max():.3e}")
    assert delta <= tol
    if mode == "fixed10":
        assert np.array_equal(iters, riters)
        assert np.abs(zncc - rzncc).max() <= 1e-9             # 225-term sums at positions that agree to 1e-12 px


def test_nonfinite_track_leaves_its_workgroup_alone():
    """The finite tracks of the non-finite case give the same bits when they are run without the others."""
    c = C.lk_cases()["nonfinite"]
    pyr = klt.build_pyramid(D(c["frames"]), c["levels"])
    keep = np.isfinite(c["points"]).all(1) & np.isfinite(c["guess"]).all(1)
    full = klt.track_pair(pyr, 0, 1, D(c["points"]), D(c["guess"]), **c["kw"])
    part = klt.track_pair(pyr, 0, 1, D(c["points"][keep]), D(c["guess"][keep]), **c["kw"])
    assert keep.sum() == 3
    for a, b in zip(full, part):
        assert a.cpu().numpy()[keep].tobytes() == b.cpu().numpy().tobytes()


def test_no_tracks_is_a_no_op():
    pyr = klt.build_pyramid(D(C.lk_cases()["flat"]["frames"]), 2)
    pos, status, zncc, iters = klt.track_pair(pyr, 0, 1, torch.zeros(0, 2, dtype=torch.float64, device="cuda"))
    assert pos.shape == (0, 2) and status.shape == zncc.shape == iters.shape == (0,)
    with pytest.raises(RuntimeError, match="invalid argument"):
        klt.track_pair(pyr, 0, 1, torch.ones(1, 2, dtype=torch.float64, device="cuda"), radius=8)


def test_determinism_and_permutation():
    """The same call twice, and the same tracks in permuted order: identical bits per track."""
    c = C.lk_cases()["n37_r7_l3"]
    pyr = klt.build_pyramid(D(c["frames"]), 3)
    a = [t.cpu().numpy() for t in klt.track_pair(pyr, 0, 1, D(c["points"]), D(c["guess"]), radius=7)]
    b = [t.cpu().numpy() for t in klt.track_pair(pyr, 0, 1, D(c["points"]), D(c["guess"]), radius=7)]
    perm = np.random.default_rng(0).permutation(37)
    p = [t.cpu().numpy() for t in klt.track_pair(pyr, 0, 1, D(c["points"][perm]), D(c["guess"][perm]), radius=7)]
    for x, y, z in zip(a, b, p):
        assert x.tobytes() == y.tobytes() and x[perm].tobytes() == z.tobytes()


# ------------------------------------------------------------------------------------------------------------ track_features
def test_visibility_of_a_blob_that_disappears_and_returns():
    """3 frames of a sparse scene moving by (2, 1) px per frame; blob 0 is absent from the middle frame."""
    centres, amp, sig = C.blob_scene(96, 128, 6, seed=4, margin=20.0, min_dist=24.0)
    step = np.array([2.0, 1.0])
    frames = []
    for f in range(3):
        keep = np.arange(6) != 0 if f == 1 else np.ones(6, bool)
        frames.append(C.render_blobs(96, 128, (centres + f * step)[keep], amp[keep], sig[keep]))
    frames = np.stack(frames)[:, None]
    track, vis, score = klt.track_features(D(frames), D(centres), query_frame=0)
    track, vis, score = track.cpu().numpy()[0], vis.cpu().numpy()[0], score.cpu().numpy()[0]
    assert track.shape == (3, 6, 2) and track.dtype == vis.dtype == score.dtype == np.float32
    assert vis[1, 0] == 0 and vis[2, 0] == 1 and (vis[:, 1:] == 1).all() and (vis[0] == 1).all() and (score[0] == 1).all()
    assert score[:, 1:].min() >= 0.9 and score[2, 0] >= 0.9
    seen = vis.astype(bool)
    truth = centres[None] + np.arange(3)[:, None, None] * step
    assert np.abs(track - truth)[seen].max() <= 0.1


def test_track_features_against_truth_and_restatement():
    """6 frames of 96 x 128 under pure translation, 12 px in all: every track within 0.1 px of truth; and, at epsilon = 0
    with 10 iterations, the chain of the first 10 tracks -- the kernel's float64 positions of all 6 frames, each search started
    from the kernel's own previous result -- within 100 x the order spread of the restatement's chained result (the spread
    measured on this chain and on the LK cases, the larger of the two)."""
    frames, centres, shifts = C.sequence_case()
    track, vis, score = (t.cpu().numpy()[0] for t in klt.track_features(D(frames), D(centres)))
    err = np.hypot(*(track - (centres[None] + shifts[:, None])).transpose(2, 0, 1))
    print(f"\nmax error against truth {err.max():.4f} px")
    assert vis.all() and err.max() <= 0.1 and score.min() >= 0.9
    fixed = C.MODES["fixed10"]
    got = [t.cpu().numpy() for t in klt._track_range64(klt.build_pyramid(D(frames), 3), 0, 6, D(centres[:10]), 0, 1.0, 0.5, fixed)]
    a = C.track_features(frames, centres[:10], **fixed)
    b = C.track_features(frames, centres[:10], reverse=True, **fixed)
    spread = max(np.abs(a[0] - b[0]).max(), C.lk_order_spread())
    delta = np.abs(got[0] - a[0]).max(axis=(1, 2))
    print(f"chain: order spread {np.abs(a[0] - b[0]).max():.3e}, |kernel - restatement| per frame {delta}")
    assert got[0].dtype == np.float64 and got[0].shape == (6, 10, 2)
    assert np.array_equal(got[1], a[1]) and a[1].all()
    assert delta.max() <= 100 * spread
    assert np.abs(got[2] - a[2]).max() <= 1e-9


def test_tracker_object_serves_predict_tracks_and_the_extra_tracker_callback():
    """KLTTracker over the 6-frame sequence: predict_tracks = detect_features + track_features; extra_tracker over the
    frames [1, 5) from frame 2 = track_features on those frames alone, bit for bit (the pyramid is per frame)."""
    frames, centres, shifts = C.sequence_case()
    dev = D(frames)
    tracker = klt.KLTTracker(dev[None], levels=3, radius=7)
    track, vis, score = tracker.predict_tracks(query_frame=0, max_query_pts=40)
    pts = klt.detect_features(dev, 0, 40)
    want = klt.track_features(dev, pts, query_frame=0, levels=3, radius=7)
    n = pts.shape[0]                                           # (the frame has fewer strict maxima than were asked for)
    assert 25 <= n <= 40 and track.shape == (1, 6, n, 2) and vis.shape == score.shape == (1, 6, n)
    assert all(torch.equal(a, b) for a, b in zip((track, vis, score), want))
    motion = (track[0, -1] - track[0, 0]).cpu().numpy()[vis[0, -1].cpu().numpy() == 1]
    assert len(motion) >= 20 and np.abs(motion - shifts[-1]).max() <= 0.1       # corners sit on the blobs' flanks: same motion
    grid = D(centres[:7] + shifts[2])[None]
    got = tracker.extra_tracker(2, 1, 5, grid)
    want = klt.track_features(dev[1:5], grid[0], query_frame=1, levels=3, radius=7)
    assert got[0].shape == (1, 4, 7, 2) and all(torch.equal(a, b) for a, b in zip(got, want))
    assert bool((got[1] == 1).all())
