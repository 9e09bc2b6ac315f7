"""GPU parity: the HIP Levenberg-Marquardt bundle adjustment (through the C-ABI) vs the Ceres/COLMAP
restatement in oracle/ba_oracle.c on identical seeded inputs.
Bar (BASELINE.json north_star): camera poses and 3D points within 1e-4 relative -- these tests use
much tighter bounds because both sides are fp64 and follow the same LM trajectory."""

import numpy as np
import pytest
import torch

from oracle import ba as OB
from vggsfm_amd import _lib
from vggsfm_amd import ba as BA
from vggsfm_amd.ba_options import BundleAdjustmentOptions
from vggsfm_amd.scene import make_scene, perturb_for_ba
from vggsfm_amd.utils.triangulation_helpers import prepare_ba_options

pytestmark = pytest.mark.gpu


def D(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


_KEEP = []        # workspaces handed to asynchronous launches stay referenced (a temporary would be freed -- and could be
#                   re-used by the next allocation -- before the kernels have run)


def _chol_ws(n):
    ws = torch.empty(int(_lib.lib().vgg_cholesky_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    _KEEP.append(ws)
    del _KEEP[:-4]
    return ws


@pytest.mark.parametrize("n", [1, 5, 32, 33, 100, 256, 257, 350, 384, 1202])
def test_cholesky_solve(n):
    rng = np.random.default_rng(n)
    M = rng.normal(size=(n, n + 8))
    A = M @ M.T + 1e-3 * np.eye(n)
    b = rng.normal(size=n)
    # asymmetric garbage in the strict upper triangle must be ignored
    Ad = np.tril(A) + np.triu(rng.normal(size=(n, n)), 1)
    At, bt = D(Ad), D(b)
    fail = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = _lib.lib().vgg_cholesky_solve(At, bt, n, _chol_ws(n), fail, _lib.stream_ptr())
    assert rc == 0
    x = bt.cpu().numpy()
    assert int(fail.item()) == 0
    xr = np.linalg.solve(A, b)
    np.testing.assert_allclose(x, xr, rtol=1e-8, atol=1e-10 * np.abs(xr).max())
    Lr = np.linalg.cholesky(A)
    np.testing.assert_allclose(np.tril(At.cpu().numpy()), Lr, rtol=1e-9, atol=1e-11)


@pytest.mark.parametrize("n", [7, 42, 64, 65, 66, 96, 102, 127, 128, 257, 350, 384, 1202, 3200, 4500])
def test_cholesky_solve_fused_rhs_row(n):
    # b stored directly behind A: the rhs rides through the factorisation as row n (the BA path)
    rng = np.random.default_rng(100 + n)
    M = rng.normal(size=(n, n + 8))
    A = M @ M.T + 1e-3 * np.eye(n)
    b = rng.normal(size=n)
    buf = D(np.concatenate([np.tril(A).ravel(), b]))
    fail = torch.zeros(1, dtype=torch.int32, device="cuda")
    At, bt = buf[:n * n], buf[n * n:]
    rc = _lib.lib().vgg_cholesky_solve(At, bt, n, _chol_ws(n), fail, _lib.stream_ptr())
    assert rc == 0 and int(fail.item()) == 0
    xr = np.linalg.solve(A, b)
    np.testing.assert_allclose(bt.cpu().numpy(), xr, rtol=1e-8, atol=1e-10 * np.abs(xr).max())


@pytest.mark.parametrize("n,sa,sb", [(1202, 384, 336), (700, 192, 256), (520, 256, 128), (450, 64, 300), (300, 128, 64)])
def test_cholesky_solve_split_matches_plain(n, sa, sb):
    """Block-diagonal leading part (no coupling between the column sets [0, sa) and [sa, sa + sb)): the two
    factorisations advance in shared panel launches.  Same L and same solution as LAPACK, and as the plain entry on the
    same matrix to rounding (the trailing updates of the two blocks reach the shared rows in a different order)."""
    rng = np.random.default_rng(n + sa)
    Lt = np.tril(rng.normal(size=(n, n))) * 0.05                    # A = Lt Lt^T with Lt[B rows][A cols] = 0 => A[B][A] = 0 exactly
    Lt[np.arange(n), np.arange(n)] = rng.uniform(1.0, 2.0, n)
    Lt[sa:sa + sb, :sa] = 0.0
    A = Lt @ Lt.T
    A[sa:sa + sb, :sa] = 0.0                                        # (sums of exact zeros; spelled out)
    A[:sa, sa:sa + sb] = 0.0
    b = rng.normal(size=n)
    out = []
    for split in (True, False):
        buf = D(np.concatenate([np.tril(A).ravel(), b]))
        fail = torch.zeros(1, dtype=torch.int32, device="cuda")
        At, bt = buf[:n * n], buf[n * n:]
        if split:
            rc = _lib.lib().vgg_cholesky_solve_split(At, bt, n, sa, sb, _chol_ws(n), fail, _lib.stream_ptr())
        else:
            rc = _lib.lib().vgg_cholesky_solve(At, bt, n, _chol_ws(n), fail, _lib.stream_ptr())
        assert rc == 0 and int(fail.item()) == 0
        out.append((np.tril(At.cpu().numpy().reshape(n, n)), bt.cpu().numpy()))
    xr = np.linalg.solve(A, b)
    np.testing.assert_allclose(out[0][1], xr, rtol=1e-8, atol=1e-10 * np.abs(xr).max())
    np.testing.assert_allclose(out[0][0], np.linalg.cholesky(A), rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(out[0][1], out[1][1], rtol=1e-10, atol=1e-13)


@pytest.mark.parametrize("n,band,arrow", [(1202, 300, 2), (2000, 200, 130), (900, 100, 0), (6002, 384, 2)])
def test_cholesky_envelope_matches_lapack(n, band, arrow):
    """Dataflow factorisation with a row envelope (vgg_ba_problem.chol_first_blk): banded matrix + dense last rows
    (the shared-intrinsics arrow) in a NESTED-DISSECTION order -- interior runs first, separators last -- so that the
    envelope has several independent leading blocks.  Same factor and solution as LAPACK on the full matrix."""
    rng = np.random.default_rng(n)
    nb = n - arrow
    M = np.zeros((n, n))
    for i in range(nb):
        lo = max(0, i - band)
        M[i, lo:i] = rng.normal(size=i - lo) * 0.05
    if arrow:
        M[nb:, :] = np.tril(rng.normal(size=(arrow, n)) * 0.05)
    A = M + M.T
    A[np.arange(n), np.arange(n)] = np.abs(A).sum(1) + 1.0
    k = max(2, min(5, nb // (3 * band)))
    rem = nb - (k - 1) * band
    sizes = [rem // k + (1 if j < rem % k else 0) for j in range(k)]
    interiors, seps, pos = [], [], 0
    for j in range(k):
        interiors += list(range(pos, pos + sizes[j]))
        pos += sizes[j]
        if j < k - 1:
            seps += list(range(pos, pos + band))
            pos += band
    order = np.array(interiors + seps + list(range(nb, n)))
    Ap = A[order][:, order]
    first_col = np.array([np.nonzero(Ap[i, :i + 1])[0][0] for i in range(n)])
    nbk = (n + 63) // 64
    fc = np.concatenate([first_col, np.full(nbk * 64 - n, n)])
    first_blk = (fc.reshape(nbk, 64).min(1) // 64).astype(np.int32)
    assert (first_blk[1:nbk - 1] > 0).any()                         # the envelope is not trivially dense
    b = rng.normal(size=n)
    buf = D(np.concatenate([np.tril(Ap).ravel(), b]))
    fail = torch.zeros(1, dtype=torch.int32, device="cuda")
    At, bt = buf[:n * n], buf[n * n:]
    fb_dev, ws = D(first_blk), _chol_ws(n)           # (kept alive until the launches have run: the call is asynchronous)
    rc = _lib.lib().vgg_cholesky_solve_envelope(At, bt, n, fb_dev, ws, fail, _lib.stream_ptr())
    assert rc == 0 and int(fail.item()) == 0
    xr = np.linalg.solve(Ap, b)
    np.testing.assert_allclose(bt.cpu().numpy(), xr, rtol=1e-8, atol=1e-10 * np.abs(xr).max())
    np.testing.assert_allclose(np.tril(At.cpu().numpy().reshape(n, n)), np.linalg.cholesky(Ap), rtol=1e-9, atol=1e-11)
    # the launch order the device derived from the envelope (df_tile_map_kernel; behind the T blocks and the flags in the
    # workspace) is the host model's, whose wait graph tests/test_chol_schedule_model.py checks
    from tests.test_chol_schedule_model import first_of_factory, tile_map
    words = ws.cpu().numpy().view(np.int32)
    base = nbk * 64 * 64 * 2 + (nbk + 1) * nbk + 3 * nbk               # T blocks | ready, tready, xready, dready | map
    chain = nbk <= 64                                                # (enqueue_dataflow: chained up to 64 block columns)
    want = tile_map(nbk, first_of_factory(nbk, first_blk), chain)
    assert int(words[base]) == len(want)
    got = words[base + 1: base + 1 + len(want)]
    assert [(int(e) & 0xffff, int(e) >> 16) for e in got] == want


def test_ba_kway_camera_order_matches_frame_order(monkeypatch):
    """Video-like visibility (tracks of at most 30 of 640 frames): compile_problem orders the cameras [interior runs,
    separators] (ba.find_camera_order) and hands the row envelope to the dataflow factorisation.  Same trajectory as
    the solve in frame order, outputs in the order of the input frames."""
    sc = make_scene(640, 14000, "SIMPLE_RADIAL", shared_camera=True, seed=29)
    first = np.argmax(sc.mask, axis=0)
    cut = np.arange(640)[:, None] >= (first + 30)[None]
    sc.mask[cut] = False
    sc.vis[cut] = 0.0
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=29)
    perm, fg = BA.find_camera_order(D(sc.mask))
    assert perm is not None and int((fg == torch.arange(len(fg))).sum()) >= 3          # >= 3 independent leading blocks
    opt = BundleAdjustmentOptions()
    opt.solver_options.max_num_iterations = 10

    def solve():
        return BA.bundle_adjustment(D(pts0), D(ext0), D(K0), D(sc.tracks), D(sc.mask), None, D(extra0), True, "SIMPLE_RADIAL", opt)
    a = solve()
    monkeypatch.setattr(BA, "find_camera_order", lambda *x, **k: (None, None))
    monkeypatch.setattr(BA, "CAMERA_SPLIT_MIN_STEPS", 10 ** 6)
    ref = solve()
    assert a[4]["num_iterations"] == ref[4]["num_iterations"]
    assert abs(a[4]["final_cost"] - ref[4]["final_cost"]) <= 1e-9 * ref[4]["final_cost"]
    for x, y in zip(a[:4], ref[:4]):
        np.testing.assert_allclose(x.cpu().numpy(), y.cpu().numpy(), rtol=1e-7, atol=1e-7)
    np.testing.assert_array_equal(a[1][0].cpu().numpy(), ext0[0])


@pytest.mark.parametrize("density_cut", [0.05, 2.0])    # compile_problem: grid filtered in place / observation list
@pytest.mark.parametrize("shared,N", [(True, 8000), (False, 5000)])
def test_ba_camera_split_matches_unsplit(monkeypatch, shared, N, density_cut):
    """Sliding-window visibility at 160 frames: bundle_adjustment orders the cameras [A, B, rest] and factorises A and B
    side by side.  Against the same solve without the re-ordering: same trajectory to rounding (the summation order of
    the reduced system changes), outputs in the order of the input frames."""
    sc = make_scene(160, N, "SIMPLE_RADIAL", shared_camera=shared, seed=13)
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=13)
    assert BA.find_camera_split(D(sc.mask))[0] is not None
    monkeypatch.setattr(BA, "SPARSE_GRID_DENSITY", density_cut)
    monkeypatch.setattr(BA, "SMALL_GRID_CELLS", 0)
    opt = BundleAdjustmentOptions()
    opt.solver_options.max_num_iterations = 12

    def solve():
        return BA.bundle_adjustment(D(pts0), D(ext0), D(K0), D(sc.tracks), D(sc.mask), None, D(extra0), shared, "SIMPLE_RADIAL", opt)
    a = solve()
    monkeypatch.setattr(BA, "CAMERA_SPLIT_MIN_STEPS", 10 ** 6)
    ref = solve()
    assert a[4]["num_iterations"] == ref[4]["num_iterations"]
    assert abs(a[4]["final_cost"] - ref[4]["final_cost"]) <= 1e-9 * ref[4]["final_cost"]
    for x, y in zip(a[:4], ref[:4]):
        np.testing.assert_allclose(x.cpu().numpy(), y.cpu().numpy(), rtol=1e-7, atol=1e-7)
    np.testing.assert_array_equal(a[1][0].cpu().numpy(), ext0[0])             # the gauge frame is still frame 0


@pytest.mark.parametrize("S,N,cam,shared", [(60, 3000, "SIMPLE_RADIAL", True), (24, 1500, "SIMPLE_PINHOLE", False), (90, 2500, "SIMPLE_RADIAL", False)])
def test_ba_launch_variants_agree(S, N, cam, shared):
    """Every launch variant of the observation passes (vgg_ba_tuning: 8 / 16 / 32 / 64 lanes per point, the long-track
    versions with four prefetched observations and no cached Jacobians, other workgroup counts of the camera and point
    passes) computes the same LM iteration up to the order of its sums: same trajectory as the automatic choice."""
    sc = make_scene(S, N, cam, shared_camera=shared, seed=23)
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=23)
    opt = BundleAdjustmentOptions()
    opt.solver_options.max_num_iterations = 8
    L = _lib.lib()

    def solve():
        return BA.bundle_adjustment(D(pts0), D(ext0), D(K0), D(sc.tracks), D(sc.mask), None, D(extra0), shared, cam, opt)
    try:
        assert L.vgg_ba_tuning(0, -1, 0, 0) == 0
        ref = solve()
        for lpp, longt, cw, pw in [(8, 0, 0, 0), (8, 1, 0, 0), (16, 0, 0, 0), (16, 1, 0, 0), (32, 0, 0, 0), (32, 1, 300, 64),
                                   (64, 0, 0, 0), (64, 1, 2048, 2048), (0, -1, 128, 7)]:
            assert L.vgg_ba_tuning(lpp, longt, cw, pw) == 0
            a = solve()
            assert a[4]["num_iterations"] == ref[4]["num_iterations"], (lpp, longt)
            assert abs(a[4]["final_cost"] - ref[4]["final_cost"]) <= 1e-9 * ref[4]["final_cost"], (lpp, longt)
            for x, y in zip(a[:4], ref[:4]):
                if x is not None:
                    np.testing.assert_allclose(x.cpu().numpy(), y.cpu().numpy(), rtol=1e-7, atol=1e-7, err_msg=str((lpp, longt, cw, pw)))
        assert L.vgg_ba_tuning(5, 0, 0, 0) != 0                          # not a lane count
    finally:
        L.vgg_ba_tuning(0, -1, 0, 0)


@pytest.mark.parametrize("S,N,cam,shared,rf,rk", [(60, 3000, "SIMPLE_RADIAL", True, True, True), (40, 2500, "SIMPLE_PINHOLE", True, True, True),
                                                  (24, 1500, "SIMPLE_RADIAL", True, True, False), (90, 2500, "SIMPLE_RADIAL", False, False, False),
                                                  (200, 12000, "SIMPLE_RADIAL", True, True, True)])
def test_ba_tile_rhs_matches_camera_pass(S, N, cam, shared, rf, rk):
    """Round 4: with 6 x 6 tile blocks the reduced right-hand side F^T (r - E h) and the shared-intrinsics border come out
    of the diagonal Schur tile launch (segments x a 3 x 3 per-point block, + per-point sums of the point pass) instead of
    a second camera-major evaluation of every projection (cam_pass<RHS>).  Same system up to the order of its sums: same
    LM trajectory as the camera pass (vgg_ba_set_tile_rhs(0)), whatever subset of the intrinsics is refined; the
    trajectory tests against the oracle run with the default (1)."""
    sc = make_scene(S, N, cam, shared_camera=shared, seed=41)
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=41)
    opt = BundleAdjustmentOptions()
    opt.refine_focal_length, opt.refine_extra_params = rf, rk
    opt.solver_options.max_num_iterations = 10
    L = _lib.lib()

    def solve():
        return BA.bundle_adjustment(D(pts0), D(ext0), D(K0), D(sc.tracks), D(sc.mask), None, D(extra0), shared, cam, opt)
    try:
        assert L.vgg_ba_set_tile_rhs(0) == 0
        ref = solve()
        assert L.vgg_ba_set_tile_rhs(1) == 0
        a, b = solve(), solve()
    finally:
        L.vgg_ba_set_tile_rhs(2)
    for x, y in zip(a[:4], b[:4]):                       # bit-reproducible
        assert x is None or torch.equal(x, y)
    assert a[4]["num_iterations"] == ref[4]["num_iterations"]
    for ia, ib in zip(a[4]["iterations"], ref[4]["iterations"]):
        assert ia["successful"] == ib["successful"] and abs(ia["cost"] - ib["cost"]) <= 1e-10 * ib["cost"], (ia, ib)
        assert abs(ia["radius"] - ib["radius"]) <= 1e-5 * ib["radius"]      # (the radius update amplifies the step quality's last bits)
    for x, y in zip(a[:4], ref[:4]):
        if x is not None:
            np.testing.assert_allclose(x.cpu().numpy(), y.cpu().numpy(), rtol=1e-8, atol=1e-8)


@pytest.mark.parametrize("S,N,cam,rf,rk,merged", [(90, 2500, "SIMPLE_RADIAL", True, True, True), (90, 2500, "SIMPLE_RADIAL", True, True, False),
                                                  (60, 3000, "SIMPLE_PINHOLE", True, False, False), (40, 2000, "SIMPLE_RADIAL", False, True, False),
                                                  (200, 8000, "SIMPLE_RADIAL", True, True, False)])
def test_ba_tile_rhs_with_per_camera_intrinsics_matches_camera_pass(S, N, cam, rf, rk, merged, monkeypatch):
    """Round 6: with PER-CAMERA intrinsics (7 x 7 / 8 x 8 tile blocks, full Schur factors) the reduced right-hand side comes out
    of the diagonal tile launch as well (vgg_ba_set_tile_rhs(2)): every thread adds the products of one tile row for two of a
    batch's four entries once the batch is in LDS; cam_pass<RHS> is not launched.  Same system up to the order of its sums:
    same LM trajectory as the camera pass, with both tile launches and with the merged one."""
    if not merged:
        monkeypatch.setattr(BA, "MERGED_TILE_MAX_OBS", 0)
    sc = make_scene(S, N, cam, shared_camera=False, seed=59)
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=59)
    opt = BundleAdjustmentOptions()
    opt.refine_focal_length, opt.refine_extra_params = rf, rk
    opt.solver_options.max_num_iterations = 10
    L = _lib.lib()

    def solve():
        return BA.bundle_adjustment(D(pts0), D(ext0), D(K0), D(sc.tracks), D(sc.mask), None, D(extra0), False, cam, opt)
    try:
        assert L.vgg_ba_set_tile_rhs(0) == 0
        ref = solve()
        assert L.vgg_ba_set_tile_rhs(2) == 0
        a, b = solve(), solve()
    finally:
        L.vgg_ba_set_tile_rhs(2)
    for x, y in zip(a[:4], b[:4]):                       # bit-reproducible
        assert x is None or torch.equal(x, y)
    assert a[4]["num_iterations"] == ref[4]["num_iterations"]
    for ia, ib in zip(a[4]["iterations"], ref[4]["iterations"]):
        assert ia["successful"] == ib["successful"] and abs(ia["cost"] - ib["cost"]) <= 1e-10 * ib["cost"], (ia, ib)
    for x, y in zip(a[:4], ref[:4]):
        if x is not None:
            np.testing.assert_allclose(x.cpu().numpy(), y.cpu().numpy(), rtol=1e-8, atol=1e-8)


def test_cholesky_flags_indefinite():
    A = np.eye(40)
    A[17, 17] = -1.0
    At, bt = D(A), D(np.ones(40))
    fail = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.lib().vgg_cholesky_solve(At, bt, 40, _chol_ws(40), fail, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert int(fail.item()) == 1


@pytest.mark.parametrize("n,pos,kind", [(200, 0, "neg"), (200, 3, "neg"), (200, 70, "neg"), (200, 199, "neg"), (350, 131, "zero"),
                                        (350, 64, "nan"), (350, 17, "inf"), (1202, 1201, "neg"), (1202, 600, "rank"),
                                        (257, 256, "neg")])
def test_cholesky_single_launch_flags_bad_pivots(n, pos, kind):
    """The single-launch factorisation (n >= 128, rhs behind the matrix: the BA path).  Round 4 took the per-pivot sign tests
    out of the 16 x 16 diagonal routine: a non-positive or non-finite pivot is caught where it surfaces -- the scale
    sqrt(d) of its column is NaN -- once per 16 columns.  Every way a pivot can be bad, at the first / an inner / the last
    column of a 4-pivot group, of a 16-block and of the ragged last 64-block: the flag must come up, and the launch must end
    (every hand-off flag is still published)."""
    rng = np.random.default_rng(n + pos)
    M = rng.normal(size=(n, n + 8))
    A = M @ M.T / n + np.eye(n)
    if kind == "neg":
        A[pos, pos] = -3.0
    elif kind == "zero":
        A[pos, :] = 0.0
        A[:, pos] = 0.0
    elif kind == "nan":
        A[pos, pos] = np.nan
    elif kind == "inf":
        A[pos, pos] = np.inf
    else:                                                 # rank deficient: row pos = row pos - 1 (pivot = rounding noise or <= 0)
        A[pos, :] = A[pos - 1, :]
        A[:, pos] = A[:, pos - 1]
        A[pos, pos] = A[pos - 1, pos - 1] - 1e-9
    buf = D(np.concatenate([np.tril(A).ravel(), rng.normal(size=n)]))
    fail = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = _lib.lib().vgg_cholesky_solve(buf[:n * n], buf[n * n:], n, _chol_ws(n), fail, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and int(fail.item()) == 1, (n, pos, kind)


CASES = [
    # S, N, camera, shared, options
    (6, 60, "SIMPLE_PINHOLE", False, "prep"),
    (8, 300, "SIMPLE_RADIAL", True, "prep"),
    (20, 400, "SIMPLE_RADIAL", False, "prep"),
    (40, 1500, "SIMPLE_PINHOLE", True, "default"),
    (50, 2000, "SIMPLE_PINHOLE", False, "prep"),
    (70, 1200, "SIMPLE_RADIAL", True, "prep"),
    (2, 200, "SIMPLE_PINHOLE", False, "prep"),       # init_BA shape: two frames
    # BASELINE configs[1] at FULL size (50 frames x 20k tracks, per-frame SIMPLE_PINHOLE, n = 350) and the camera
    # configuration of configs[2] (200 frames, shared SIMPLE_RADIAL, n = 1202) at 10k tracks: 12 LM iterations each
    # (the CPU port needs ~1 s per iteration here)
    (50, 20000, "SIMPLE_PINHOLE", False, "prep12"),
    (200, 10000, "SIMPLE_RADIAL", True, "prep12"),
    # the HEADLINE configuration, BASELINE configs[2] at full size (200 frames x 100k tracks, shared
    # SIMPLE_RADIAL, 5 M observations, n = 1202), 5 LM iterations (~2 s each for the CPU port), and the block shape of
    # configs[3] -- per-frame SIMPLE_RADIAL, 8 x 8 camera blocks, the 128 x 128 tile variant, n = 3200 -- at 400 frames
    (200, 100000, "SIMPLE_RADIAL", True, "prep5"),
    (400, 5000, "SIMPLE_RADIAL", False, "prep8"),
]


def _oracle_opts(kind):
    if kind in ("prep12", "prep8", "prep5"):
        o = OB.prepare_ba_options()
        o.max_num_iterations = int(kind[4:])
        return o
    return OB.prepare_ba_options() if kind == "prep" else OB.ceres_options()


def _gpu_opts(kind):
    if kind in ("prep12", "prep8", "prep5"):
        o = prepare_ba_options()
        o.solver_options.max_num_iterations = int(kind[4:])
        return o
    return prepare_ba_options() if kind == "prep" else BundleAdjustmentOptions()


def _compare_trajectories(sg, so, min_compared):
    """Iteration logs of the GPU solve (sg) and of the oracle (so) side by side: same accept / reject pattern, costs to
    1e-9, radii and gradient norms to 1e-5 for as long as the decisions are not made of rounding noise -- once
    |cost change| < 1e-9 * cost the step quality (cost change / model change) is noise in BOTH implementations and the
    accept / reject pattern is not comparable.  EXITS: when the oracle's whole log stays above that
    floor, the two solves must also END alike -- same termination type, same number of iterations."""
    compared, hit_floor = 0, False
    for a, b in zip(sg["iterations"], so["iterations"]):
        if b["iteration"] > 0 and abs(b["cost_change"]) < 1e-9 * b["cost"]:
            hit_floor = True
            break
        assert a["iteration"] == b["iteration"] and a["successful"] == b["successful"], (a, b)
        assert abs(a["cost"] - b["cost"]) <= 1e-9 * b["cost"], (a, b)
        assert abs(a["radius"] - b["radius"]) <= 1e-5 * b["radius"], (a, b)
        assert abs(a["gradient_max_norm"] - b["gradient_max_norm"]) <= 1e-5 * b["gradient_max_norm"] + 1e-9, (a, b)
        compared += 1
    assert compared >= min(min_compared, so["num_iterations"])
    if not hit_floor:
        assert sg["termination"] == so["termination"], (sg["termination_str"], so["termination"])
        assert sg["num_iterations"] == so["num_iterations"]
        assert len(sg["iterations"]) == len(so["iterations"])
    return compared, hit_floor


@pytest.mark.parametrize("S,N,cam,shared,kind", CASES)
def test_ba_matches_oracle_trajectory(S, N, cam, shared, kind):
    sc = make_scene(S, N, cam, shared_camera=shared, seed=S + N, full_visibility=(S <= 3))
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=S + N)
    po, eo, Ko, xo, so = OB.bundle_adjustment(pts0, ext0, K0, sc.tracks, sc.mask, extra0, shared, cam, _oracle_opts(kind))
    pts, ext, K, extra, sg = BA.bundle_adjustment(D(pts0), D(ext0), D(K0), D(sc.tracks), D(sc.mask), None, D(extra0),
                                                  shared, cam, _gpu_opts(kind))
    assert np.array_equal(sg["valid_idx"].cpu().numpy(), so["valid_idx"])
    assert sg["n_reduced"] == so["n_reduced"]
    assert abs(sg["initial_cost"] - so["initial_cost"]) <= 1e-11 * so["initial_cost"]
    _compare_trajectories(sg, so, 6)
    assert abs(sg["final_cost"] - so["final_cost"]) <= 1e-8 * so["final_cost"]
    np.testing.assert_allclose(ext.cpu().numpy(), eo, rtol=0, atol=5e-6)
    # (final values: both sides stop at the gradient tolerance, not at the exact optimum, and the last accept /
    #  reject decisions sit at the rounding-noise floor -- hence 1e-6, the north-star figure is 1e-4)
    np.testing.assert_allclose(K.cpu().numpy()[:, 0, 0], Ko[:, 0, 0], rtol=1e-6)
    np.testing.assert_allclose(pts.cpu().numpy(), po, rtol=0, atol=5e-5)
    if xo is not None:
        np.testing.assert_allclose(extra.cpu().numpy(), xo, rtol=0, atol=1e-7)
    # gauge: image 0 untouched, x-translation of image 1 untouched
    np.testing.assert_allclose(ext.cpu().numpy()[0], ext0[0], atol=1e-15)
    assert float(ext[1, 0, 3]) == ext0[1, 0, 3]


EXIT_CASES = [
    # solves that END on the gradient test well above the rounding-noise floor (a loose tolerance on a noisy scene): the
    # termination type and the iteration on which it fires are part of the parity claim
    # (gradient max-norms are in pixel^2 units: 1e3 .. 1e4 a few iterations in; with the reference's own 1e-3 / 1e-4 the
    #  test is only met where the cost changes by < 1e-14 of itself -- see DESIGN.md section 5, "exits")
    (12, 900, "SIMPLE_RADIAL", True, 100.0),         # oracle: iteration 15
    (30, 2500, "SIMPLE_PINHOLE", False, 2000.0),     # 5
    (70, 1200, "SIMPLE_RADIAL", True, 300.0),        # 7
    (50, 20000, "SIMPLE_PINHOLE", False, 5000.0),    # 5
    (200, 10000, "SIMPLE_RADIAL", True, 1000.0),     # 7
]


@pytest.mark.parametrize("S,N,cam,shared,gtol", EXIT_CASES)
def test_ba_exit_matches_oracle(S, N, cam, shared, gtol):
    """the gradient tolerance is reached while every decision is still far above rounding noise; GPU
    and oracle must stop on the SAME iteration with the SAME termination type (Ceres checks the gradient norm at the
    start of an iteration and only behind a successful step)."""
    sc = make_scene(S, N, cam, shared_camera=shared, seed=3 * S + N)
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=3 * S + N)
    oo = OB.ceres_options(50, 0.0, gtol, 0.0)
    go = BundleAdjustmentOptions()
    go.solver_options.max_num_iterations, go.solver_options.gradient_tolerance = 50, gtol
    po, eo, Ko, xo, so = OB.bundle_adjustment(pts0, ext0, K0, sc.tracks, sc.mask, extra0, shared, cam, oo)
    pts, ext, K, extra, sg = BA.bundle_adjustment(D(pts0), D(ext0), D(K0), D(sc.tracks), D(sc.mask), None, D(extra0),
                                                  shared, cam, go)
    compared, hit_floor = _compare_trajectories(sg, so, 2)
    assert not hit_floor, "pick a looser tolerance: the case is meant to end above the noise floor"
    assert so["termination"] == 1 and 2 <= so["num_iterations"] < 50      # CONVERGENCE (gradient tolerance), not the cap
    assert sg["termination"] == 1 and sg["num_iterations"] == so["num_iterations"]
    np.testing.assert_allclose(ext.cpu().numpy(), eo, rtol=0, atol=1e-8)
    np.testing.assert_allclose(pts.cpu().numpy(), po, rtol=0, atol=1e-7)


def _video_scene(S, N, span, seed):
    """Video-like visibility: every track ends `span` frames after it starts (vggsfm/runners/video_runner.py: a track lives
    in one window of <= 33 frames), shared SIMPLE_RADIAL camera."""
    sc = make_scene(S, N, "SIMPLE_RADIAL", shared_camera=True, seed=seed)
    first = np.argmax(sc.mask, axis=0)
    cut = np.arange(S)[:, None] >= (first + span)[None]
    sc.mask[cut] = False
    sc.vis[cut] = 0.0
    return sc


def test_ba_video_shape_matches_oracle_trajectory():
    """VERDICT r3 item 1a / missing 4: the joint BA of the video path (vggsfm/runners/video_runner.py:494-541) at its own
    shape -- 640 frames x 14 k tracks of at most 30 frames, shared SIMPLE_RADIAL, n = 3842 -- where compile_problem orders
    the cameras k-way [interior runs, separators] and the factorisation runs on the row envelope: 10 LM iterations against
    ba_oracle.c (frame order, dense Cholesky), not only against the same GPU solve in frame order."""
    sc = _video_scene(640, 14000, 30, 29)
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=29)
    perm, fg = BA.find_camera_order(D(sc.mask))
    assert perm is not None and int((fg == torch.arange(len(fg))).sum()) >= 3          # >= 3 independent leading blocks
    oo = OB.prepare_ba_options()
    oo.max_num_iterations = 10
    go = prepare_ba_options()
    go.solver_options.max_num_iterations = 10
    po, eo, Ko, xo, so = OB.bundle_adjustment(pts0, ext0, K0, sc.tracks, sc.mask, extra0, True, "SIMPLE_RADIAL", oo)
    pts, ext, K, extra, sg = BA.bundle_adjustment(D(pts0), D(ext0), D(K0), D(sc.tracks), D(sc.mask), None, D(extra0),
                                                  True, "SIMPLE_RADIAL", go)
    assert np.array_equal(sg["valid_idx"].cpu().numpy(), so["valid_idx"]) and sg["n_reduced"] == so["n_reduced"] == 3842
    compared, _ = _compare_trajectories(sg, so, 8)
    assert abs(sg["final_cost"] - so["final_cost"]) <= 1e-8 * so["final_cost"]
    np.testing.assert_allclose(ext.cpu().numpy(), eo, rtol=0, atol=5e-6)        # (in the order of the INPUT frames)
    np.testing.assert_allclose(pts.cpu().numpy(), po, rtol=0, atol=5e-5)
    np.testing.assert_allclose(float(K[0, 0, 0]), Ko[0, 0, 0], rtol=1e-6)
    np.testing.assert_allclose(extra.cpu().numpy(), xo, rtol=0, atol=1e-7)


def test_ba_deleted_points_and_constant_blocks():
    sc = make_scene(5, 80, "SIMPLE_PINHOLE", seed=4, full_visibility=True, outlier_frac=0.0)
    ext0, K0, _, pts0 = perturb_for_ba(sc, seed=4)
    masks = sc.mask.copy()
    masks[2:, 0] = False
    pts0[0] = [0.0, 0.0, -3.0]
    pts0[1, 2] = 3500.0
    po, eo, Ko, xo, so = OB.bundle_adjustment(pts0, ext0, K0, sc.tracks, masks, None, False, "SIMPLE_PINHOLE",
                                              OB.prepare_ba_options())
    pts, ext, K, extra, sg = BA.bundle_adjustment(D(pts0), D(ext0), D(K0), D(sc.tracks), D(masks), None, None, False,
                                                  "SIMPLE_PINHOLE", prepare_ba_options())
    assert np.array_equal(sg["deleted"].cpu().numpy(), so["deleted"])
    np.testing.assert_allclose(pts.cpu().numpy(), po, atol=1e-6)
    np.testing.assert_allclose(ext.cpu().numpy(), eo, atol=1e-7)
    assert (pts[0] == 0).all() and np.array_equal(pts[1].cpu().numpy(), pts0[1])


def test_ba_converges_to_ground_truth_without_noise():
    # property at a size the oracle would need minutes for: noise-free observations -> BA drives the
    # cost to ~0 and recovers the ground-truth cameras (gauge is fixed by image 0 / t_x of image 1)
    sc = make_scene(60, 20000, "SIMPLE_RADIAL", shared_camera=True, seed=8, noise_px=0.0, outlier_frac=0.0)
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=8)
    ext0[1, 0, 3] = sc.extrinsics[1, 0, 3]          # the gauge-fixed coordinate must already be right
    opt = BundleAdjustmentOptions()
    opt.solver_options.gradient_tolerance = 1e-10
    pts, ext, K, extra, sg = BA.bundle_adjustment(D(pts0), D(ext0), D(K0), D(sc.tracks), D(sc.mask), None, D(extra0),
                                                  True, "SIMPLE_RADIAL", opt)
    assert sg["final_cost"] < 1e-3 * sg["initial_cost"]
    # float32 storage of the observations bounds the residual: ~3e-5 px
    assert sg["final_cost"] / (2 * int(sc.mask.sum())) < 1e-8
    np.testing.assert_allclose(ext.cpu().numpy(), sc.extrinsics, atol=2e-6)
    np.testing.assert_allclose(pts.cpu().numpy(), sc.points3D, atol=1e-5)
    np.testing.assert_allclose(float(K[0, 0, 0]), 1000.0, rtol=1e-6)


@pytest.mark.parametrize("cam,shared,S,N,n_exist", [("SIMPLE_RADIAL", True, 17, 900, 500), ("SIMPLE_PINHOLE", True, 17, 900, 500),
                                                     # the INITIAL window of the video runner: 2 x window_size + 1 frames
                                                     # (vggsfm/runners/video_runner.py:200-230), 2 x 1024 new tracks
                                                     ("SIMPLE_RADIAL", True, 33, 4000, 1900)])
def test_window_bundle_adjustment_matches_oracle(cam, shared, S, N, n_exist):
    """Local BA of a video window (vggsfm/runners/video_runner.py:800-838): frame 0 constant, carried-over points
    constant, new points variable, intrinsics not refined, no negative-depth filter."""
    # window_size + 1 (or 2 x window_size + 1) frames; existing + newly triangulated tracks
    sc = make_scene(S, N, cam, shared_camera=shared, seed=12, full_visibility=False, outlier_frac=0.0)
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=12)
    ext0[0] = sc.extrinsics[0]
    valid = sc.mask.sum(0) >= 2
    order = np.cumsum(valid) - 1
    constant = valid & (order < n_exist)
    pts0[constant] = sc.points3D[constant]          # carried-over points are already refined
    oo = OB.ceres_options(100)
    po, eo, Ko, xo, so = OB.bundle_adjustment(pts0, ext0, K0, sc.tracks, sc.mask, extra0, shared, cam, options=oo,
                                              constant_points=constant, constant_pose_frames=[0],
                                              filter_negative_depth=False, refine_focal=False, refine_extra=False)
    pts, ext, K, extra, sg = BA.window_bundle_adjustment(D(pts0), D(ext0), D(K0), D(sc.tracks), D(sc.mask), n_exist,
                                                         D(extra0), shared, cam)
    # same trajectory while the cost change is above the rounding-noise floor (below it the accept / reject
    # decision of the two implementations is a coin toss, cf. test_ba_matches_oracle_trajectory)
    for a, b in zip(so["iterations"], sg["iterations"]):
        if a["iteration"] > 0 and abs(a["cost_change"]) < 1e-9 * a["cost"]:
            break
        assert a["successful"] == b["successful"]
        np.testing.assert_allclose(b["cost"], a["cost"], rtol=1e-9)
        np.testing.assert_allclose(b["radius"], a["radius"], rtol=1e-5)
    np.testing.assert_allclose(sg["final_cost"], so["final_cost"], rtol=1e-9)
    vi = so["valid_idx"]
    # constant blocks did not move at all; intrinsics untouched
    assert np.array_equal(pts.cpu().numpy()[constant[vi]], pts0[vi][constant[vi]])
    assert np.array_equal(ext[0].cpu().numpy(), ext0[0]) and np.array_equal(K.cpu().numpy(), K0)
    np.testing.assert_allclose(pts.cpu().numpy(), po, atol=2e-6)
    np.testing.assert_allclose(ext.cpu().numpy(), eo, atol=1e-7)
    assert sg["final_cost"] < 0.2 * sg["initial_cost"]


def test_ba_full_size_c3_properties():
    """BASELINE configs[2] at full size (200 frames x 100k tracks, SIMPLE_RADIAL, shared camera; ~5 M observations, far
    beyond what the oracle finishes in seconds): size-independent properties.  Noise-free observations of the
    ground-truth scene => BA must drive the cost to the float32-storage floor of the pixels and recover the
    ground-truth cameras / points / intrinsics from a perturbed start (the gauge is fixed by image 0 and t_x of
    image 1, both left at their ground-truth values)."""
    sc = make_scene(200, 100000, "SIMPLE_RADIAL", shared_camera=True, seed=0, noise_px=0.0, outlier_frac=0.0)
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=0)
    ext0[0] = sc.extrinsics[0]
    ext0[1, 0, 3] = sc.extrinsics[1, 0, 3]
    opt = BundleAdjustmentOptions()
    opt.solver_options.gradient_tolerance = 1e-10
    opt.solver_options.max_num_iterations = 40
    pts, ext, K, extra, sg = BA.bundle_adjustment(D(pts0), D(ext0), D(K0), D(sc.tracks), D(sc.mask), None, D(extra0),
                                                  True, "SIMPLE_RADIAL", opt)
    n_res = 2 * int(sc.mask[:, sc.mask.sum(0) >= 2].sum())
    assert sg["n_reduced"] == 6 * 200 + 2
    assert sg["final_cost"] < 1e-6 * sg["initial_cost"]
    assert sg["final_cost"] / n_res < 1e-8                       # ~3e-5 px rms: float32 pixels
    # monotone cost over the successful steps (Levenberg-Marquardt invariant)
    costs = [it["cost"] for it in sg["iterations"] if it["successful"]]
    assert all(b <= a * (1 + 1e-12) for a, b in zip(costs, costs[1:]))
    # (accuracy floor: the observations are stored in float32, 3e-5 px)
    np.testing.assert_allclose(ext.cpu().numpy(), sc.extrinsics, atol=2e-5)
    vi = sg["valid_idx"].cpu().numpy()
    np.testing.assert_allclose(pts.cpu().numpy(), sc.points3D[vi], atol=1e-4)
    np.testing.assert_allclose(float(K[0, 0, 0]), 1000.0, rtol=1e-6)
    np.testing.assert_allclose(float(extra[0, 0]), sc.extra_params[0, 0], atol=1e-6)


@pytest.mark.parametrize("shared,S,N", [(True, 72, 6000), (False, 56, 4000)])
def test_ba_overlapped_factorization_matches_single_stream(monkeypatch, shared, S, N):
    """Opt-in mode (ba.OVERLAP_FACTORIZATION): Schur tiles in 3 batches, batches 1.. and the Cholesky factorisation
    on two CU-masked streams, the late batches added to the panel when it is loaded (S2).  Only the summation order
    changes: same trajectory to rounding as the single-stream solve, and bit-identical from run to run (a race
    between a batch and the panel that reads it would show up here)."""
    sc = make_scene(S, N, "SIMPLE_RADIAL", shared_camera=shared, seed=11)
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=11)
    opt = BundleAdjustmentOptions()
    opt.solver_options.max_num_iterations = 15

    def solve():
        return BA.bundle_adjustment(D(pts0), D(ext0), D(K0), D(sc.tracks), D(sc.mask), None, D(extra0), shared,
                                    "SIMPLE_RADIAL", opt)
    ref = solve()
    monkeypatch.setattr(BA, "OVERLAP_FACTORIZATION", True)
    monkeypatch.setattr(BA, "OVERLAP_MIN_OBS", 0)
    monkeypatch.setattr(BA, "OVERLAP_MIN_FRAMES", 0)
    a, b = solve(), solve()
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    assert a[4]["num_iterations"] == ref[4]["num_iterations"]
    assert abs(a[4]["final_cost"] - ref[4]["final_cost"]) <= 1e-9 * ref[4]["final_cost"]
    for x, y in zip(a[:4], ref[:4]):
        np.testing.assert_allclose(x.cpu().numpy(), y.cpu().numpy(), rtol=1e-7, atol=1e-7)


@pytest.mark.parametrize("shared,S,N", [(True, 72, 6000), (True, 160, 8000), (False, 56, 4000)])
def test_ba_default_path_is_bit_reproducible(shared, S, N):
    """No atomics and fixed summation orders anywhere in the iteration (tile chunks reduced in order, camera slices in
    order; the hand-offs of the single-launch factorisation carry data, never sums, and its update order is a function of
    the envelope): two solves of the same problem give the same bits -- cameras, points, cost trajectory.  At 160 frames
    the cameras are ordered [A, B, rest] (decoupled leading blocks: chained factorisation + depth-ordered updates)."""
    sc = make_scene(S, N, "SIMPLE_RADIAL", shared_camera=shared, seed=5)
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=5)
    opt = BundleAdjustmentOptions()
    opt.solver_options.max_num_iterations = 12

    def solve():
        return BA.bundle_adjustment(D(pts0), D(ext0), D(K0), D(sc.tracks), D(sc.mask), None, D(extra0), shared, "SIMPLE_RADIAL", opt)
    a, b = solve(), solve()
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    assert [it["cost"] for it in a[4]["iterations"]] == [it["cost"] for it in b[4]["iterations"]]
    assert a[4]["n_reduced"] >= 128                                  # (the single-launch factorisation ran)


def test_ba_per_frame_intrinsics_at_scale_properties():
    """BASELINE configs[3] shape at reduced size (per-frame focal + distortion => 8x8 camera blocks, the 128 x 128
    Schur tile variant over 8 camera groups): noise-free scene recovered from a perturbed start."""
    sc = make_scene(120, 15000, "SIMPLE_RADIAL", shared_camera=False, seed=6, noise_px=0.0, outlier_frac=0.0)
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=6)
    ext0[0] = sc.extrinsics[0]
    ext0[1, 0, 3] = sc.extrinsics[1, 0, 3]
    opt = BundleAdjustmentOptions()
    opt.solver_options.gradient_tolerance = 1e-10
    opt.solver_options.max_num_iterations = 60
    pts, ext, K, extra, sg = BA.bundle_adjustment(D(pts0), D(ext0), D(K0), D(sc.tracks), D(sc.mask), None, D(extra0),
                                                  False, "SIMPLE_RADIAL", opt)
    assert sg["n_reduced"] == 8 * 120
    assert sg["final_cost"] < 1e-6 * sg["initial_cost"]
    costs = [it["cost"] for it in sg["iterations"] if it["successful"]]
    assert all(b <= a * (1 + 1e-12) for a, b in zip(costs, costs[1:]))
    np.testing.assert_allclose(ext.cpu().numpy(), sc.extrinsics, atol=5e-5)
    np.testing.assert_allclose(K.cpu().numpy()[:, 0, 0], sc.intrinsics[:, 0, 0], rtol=2e-5)
    np.testing.assert_allclose(extra.cpu().numpy(), sc.extra_params, atol=2e-5)


@pytest.mark.parametrize("loss,scale", [("HUBER", 1.0), ("CAUCHY", 2.0), ("SOFT_L1", 1.5)])
def test_ba_robust_losses_match_oracle(loss, scale):
    """Ceres loss functions + corrector (`BundleAdjustmentOptions.loss_function_type`, COLMAP CreateLossFunction):
    Huber-weighted (and Cauchy / SoftL1) normal equations on a scene WITH outliers, GPU vs oracle."""
    from vggsfm_amd.ba_options import LOSS_ID
    sc = make_scene(12, 900, "SIMPLE_RADIAL", shared_camera=True, seed=17, outlier_frac=0.08)
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=17)
    opt = BundleAdjustmentOptions()
    opt.loss_function_type, opt.loss_function_scale = loss, scale
    opt.solver_options.max_num_iterations = 30
    oo = OB.ceres_options(30)
    po, eo, Ko, xo, so = OB.bundle_adjustment(pts0, ext0, K0, sc.tracks, sc.mask, extra0, True, "SIMPLE_RADIAL", options=oo,
                                              loss=LOSS_ID[loss], loss_scale=scale)
    pts, ext, K, extra, sg = BA.bundle_adjustment(D(pts0), D(ext0), D(K0), D(sc.tracks), D(sc.mask), None, D(extra0), True,
                                                  "SIMPLE_RADIAL", opt)
    compared = 0
    for a, b in zip(sg["iterations"], so["iterations"]):
        if b["iteration"] > 0 and abs(b["cost_change"]) < 1e-9 * b["cost"]:
            break
        assert a["successful"] == b["successful"], (a, b)
        assert abs(a["cost"] - b["cost"]) <= 1e-9 * b["cost"], (a, b)
        compared += 1
    assert compared >= 4
    # the robust cost is far below the squared cost of the same residuals (the outliers are down-weighted)
    assert abs(sg["final_cost"] - so["final_cost"]) <= 1e-8 * so["final_cost"]
    np.testing.assert_allclose(ext.cpu().numpy(), eo, atol=5e-6)
    np.testing.assert_allclose(pts.cpu().numpy(), po, atol=5e-5)
    np.testing.assert_allclose(float(K[0, 0, 0]), Ko[0, 0, 0], rtol=1e-6)


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("rf,rk", [(True, False), (False, True), (False, False)])
def test_ba_partial_intrinsics_refinement_matches_oracle(shared, rf, rk):
    """`refine_focal_length` / `refine_extra_params` combinations (COLMAP SetConstantCamIntrinsics subsets): focal
    only, distortion only (the `only_k` layout of the camera block), neither."""
    sc = make_scene(10, 700, "SIMPLE_RADIAL", shared_camera=shared, seed=19, outlier_frac=0.0)
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=19)
    opt = BundleAdjustmentOptions()
    opt.refine_focal_length, opt.refine_extra_params = rf, rk
    opt.solver_options.max_num_iterations = 25
    po, eo, Ko, xo, so = OB.bundle_adjustment(pts0, ext0, K0, sc.tracks, sc.mask, extra0, shared, "SIMPLE_RADIAL",
                                              options=OB.ceres_options(25), refine_focal=rf, refine_extra=rk)
    pts, ext, K, extra, sg = BA.bundle_adjustment(D(pts0), D(ext0), D(K0), D(sc.tracks), D(sc.mask), None, D(extra0),
                                                  shared, "SIMPLE_RADIAL", opt)
    assert sg["n_reduced"] == so["n_reduced"]
    for a, b in zip(sg["iterations"], so["iterations"]):
        if b["iteration"] > 0 and abs(b["cost_change"]) < 1e-9 * b["cost"]:
            break
        assert a["successful"] == b["successful"] and abs(a["cost"] - b["cost"]) <= 1e-9 * b["cost"], (a, b)
    assert abs(sg["final_cost"] - so["final_cost"]) <= 1e-8 * so["final_cost"]
    if not rf:
        assert np.array_equal(K.cpu().numpy(), K0)                 # focal untouched
    if not rk:
        assert np.array_equal(extra.cpu().numpy(), extra0)         # distortion untouched
    np.testing.assert_allclose(ext.cpu().numpy(), eo, atol=5e-6)
    np.testing.assert_allclose(K.cpu().numpy()[:, 0, 0], Ko[:, 0, 0], rtol=1e-6)
    np.testing.assert_allclose(extra.cpu().numpy(), xo, atol=1e-6)
