"""Every device entry on poisoned, guard-banded memory (tests/poison.py).

The parity tests run their kernels on whatever the caching allocator hands back for ``torch.empty``.  Here a
representative case of each entry -- the existing test itself, with its inputs and its reference bar -- runs with every
``empty``-family buffer filled with 0x00, 0xFF (NaN / -1) and 0x7F (huge finite) and framed by guard bands, and:
  (a) what the test reads back from the device (every ``.cpu()`` / ``.item()`` / ``.tolist()``) is bit-identical across the
      three patterns -- after two runs under one pattern have shown that the case is run-to-run deterministic;
  (b) no guard byte changed (checked when each poisoned run ends);
  (c) the existing test's own assertions against its oracle or golden hold under every pattern, 0xFF included;
  (d) no floating-point value read back is still the pattern (0xFF or 0x7F in every byte), nor any 32 / 64-bit integer
      0x7F7F... -- neither is a value the kernels produce.
Then the contracts of the multi-GPU reduce buffers (include/vggsfm_amd.h, vgg_ba_begin .. vgg_ba_reduce_buffer)."""
import hashlib
import os

import numpy as np
import pytest
import torch

import oracle.ba as OB
from tests import test_gpu_ba as TB
from tests import test_gpu_dense_depth as TDD
from tests import test_gpu_dist as TD
from tests import test_gpu_fundamental as TF
from tests import test_gpu_geometry as TG
from tests import test_gpu_p3p as TP
from tests import test_gpu_pose as TPO
from tests import test_gpu_pose_regimes as TPR
from tests import test_gpu_reproj_video as TR
from tests import test_gpu_triangulation as TT
from tests.poison import equals_pattern, poisoned_allocations
from vggsfm_amd import _lib
from vggsfm_amd import ba as BA
from vggsfm_amd.dist import ShardedBA
from vggsfm_amd.scene import make_scene, perturb_for_ba
from vggsfm_amd.utils.triangulation_helpers import prepare_ba_options

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def D(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


# --- read-back tap --------------------------------------------------------------------------------------------------
class _Tap:
    """Records a host copy of everything the test reads back from its tensors, in order."""

    def __init__(self):
        self.seen = []
        self._orig = (torch.Tensor.cpu, torch.Tensor.item, torch.Tensor.tolist)

    def __enter__(self):
        cpu, item, tolist = self._orig
        seen = self.seen

        def tap_cpu(t, *a, **k):
            r = cpu(t, *a, **k)
            seen.append(r.detach().numpy().copy())
            return r

        def tap_item(t):
            seen.append(cpu(t).detach().numpy().copy())
            return item(t)

        def tap_tolist(t):
            seen.append(cpu(t).detach().numpy().copy())
            return tolist(t)
        torch.Tensor.cpu, torch.Tensor.item, torch.Tensor.tolist = tap_cpu, tap_item, tap_tolist
        return self

    def __exit__(self, *exc):
        torch.Tensor.cpu, torch.Tensor.item, torch.Tensor.tolist = self._orig
        return False


def _run(case, pattern):
    """One poisoned run of `case(monkeypatch)`; the guards are checked when the poisoned context ends.  The global RNG is
    reseeded first: some wrappers draw host-side seeds from it (align_dense_depth_maps) even when the test fixes the samples."""
    torch.manual_seed(0)
    with poisoned_allocations(pattern) as st, pytest.MonkeyPatch.context() as mp, _Tap() as tap:
        case(mp)
    assert st.blocks == []                                  # (released after the guard check)
    return tap.seen


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _not_pattern(seen, pattern, label):
    for i, a in enumerate(seen):
        if a.dtype.kind == "f" or (pattern == 0x7F and a.dtype.kind in "iu" and a.dtype.itemsize >= 4):
            hit = equals_pattern(a, pattern)
            assert not hit.any(), f"{label}: read-back #{i} {a.shape} {a.dtype} still holds the 0x{pattern:02X} pattern " \
                                  f"at {np.argwhere(hit)[:4].tolist()}"


def _check_poisoned(case, ignore=()):
    """(a)-(d) of the module docstring for one case (the case's own assertions are (c)).  `ignore`: indices of read-backs that
    are not outputs (a whole workspace the test inspects part of)."""
    ff = _run(case, 0xFF)
    again = _run(case, 0xFF)
    assert len(ff) == len(again), "not run-to-run deterministic"
    nondet = [i for i, (x, y) in enumerate(zip(ff, again)) if i not in ignore and not _same(x, y)]
    assert not nondet, f"read-backs {nondet[:8]} are not run-to-run deterministic"
    assert len(ff) > 0, "the case read nothing back"
    for pattern in (0x00, 0x7F):
        got = _run(case, pattern)
        assert len(got) == len(ff)
        diff = [i for i, (x, y) in enumerate(zip(ff, got)) if i not in ignore and not _same(x, y)]
        assert not diff, f"read-backs {diff[:8]} differ between the 0xFF and 0x{pattern:02X} patterns " \
                         f"(first: {ff[diff[0]].shape} {ff[diff[0]].dtype})"
        if pattern == 0x7F:
            _not_pattern([a for i, a in enumerate(got) if i not in ignore], pattern, "0x7F")
    _not_pattern([a for i, a in enumerate(ff) if i not in ignore], 0xFF, "0xFF")


def _memo_oracle(monkeypatch):
    """The CPU oracle's BA is deterministic: solve each problem once for the four poisoned runs of a case."""
    cache, inner = {}, OB.bundle_adjustment

    def key(v):
        if isinstance(v, np.ndarray):
            return (v.dtype.str, v.shape, hashlib.sha1(np.ascontiguousarray(v).tobytes()).hexdigest())
        if hasattr(v, "__dict__"):
            return repr(sorted(vars(v).items()))
        return repr(v)

    def memo(*a, **k):
        kk = (tuple(key(v) for v in a), tuple((n, key(v)) for n, v in sorted(k.items())))
        if kk not in cache:
            cache[kk] = inner(*a, **k)
        po, eo, Ko, xo, so = cache[kk]
        return po.copy(), eo.copy(), Ko.copy(), None if xo is None else xo.copy(), so
    monkeypatch.setattr(OB, "bundle_adjustment", memo)


@pytest.fixture(autouse=True)
def _oracle_memo(monkeypatch):
    _memo_oracle(monkeypatch)


# --- the entries -----------------------------------------------------------------------------------------------------
def _merged_off(mp):
    mp.setattr(BA, "MERGED_TILE_MAX_OBS", 0)


def _f64_tracks(mp, module):
    """The module's golden loader with the tracks as float64 (the `tracks_are_f64` branch of the geometry kernels; the
    fp32 values are exact in fp64, so the goldens and their bars still apply)."""
    load = module._load

    def f64(golden_dir, name):
        g = load(golden_dir, name)
        g["tracks"] = g["tracks"].astype(np.float64)
        return g
    mp.setattr(module, "_load", f64)


CASES = {
    # Cholesky: separate b = the multi-launch path at every n; b behind A = the dataflow path from n = 128 (4500: 71 block
    # columns, beyond the 64 of the chained schedule); the split and the envelope entries
    **{f"chol_separate_n{n}": (lambda mp, n=n: TB.test_cholesky_solve(n)) for n in (1, 65, 127, 1202)},
    **{f"chol_fused_n{n}": (lambda mp, n=n: TB.test_cholesky_solve_fused_rhs_row(n)) for n in (65, 127, 1202, 4500)},
    "chol_split": lambda mp: TB.test_cholesky_solve_split_matches_plain(1202, 384, 336),
    "chol_envelope": lambda mp: TB.test_cholesky_envelope_matches_lapack(1202, 300, 2),
    # BA vs the oracle around the 16-camera Schur groups and the 64-column blocks (n = 6 S + 2 with shared SIMPLE_RADIAL),
    # both tile forms, per-frame SIMPLE_PINHOLE, and the configs[2] camera shape
    **{f"ba_S{S}_merged": (lambda mp, S=S: TB.test_ba_matches_oracle_trajectory(S, 40 * S + 200, "SIMPLE_RADIAL", True, "prep"))
       for S in (15, 16, 17, 33)},
    **{f"ba_S{S}_separate": (lambda mp, S=S: (_merged_off(mp), TB.test_ba_matches_oracle_trajectory(
        S, 40 * S + 200, "SIMPLE_RADIAL", True, "prep"))) for S in (17, 33)},
    "ba_per_frame_radial": lambda mp: TB.test_ba_matches_oracle_trajectory(20, 400, "SIMPLE_RADIAL", False, "prep"),
    "ba_per_frame_simple_pinhole": lambda mp: TB.test_ba_matches_oracle_trajectory(50, 2000, "SIMPLE_PINHOLE", False, "prep"),
    "ba_S200_N10000": lambda mp: TB.test_ba_matches_oracle_trajectory(200, 10000, "SIMPLE_RADIAL", True, "prep12"),
    # the sharded solve, emulated ranks: one-piece, in-place and split exchanges
    "sharded_w2_one_piece": lambda mp: TD.test_sharded_equals_single_rank("SIMPLE_RADIAL", True, 2, False, mp),
    "sharded_w3_in_place": lambda mp: TD.test_sharded_equals_single_rank("SIMPLE_PINHOLE", False, 3, True, mp),
    "sharded_w2_split": lambda mp: TD.test_sharded_equals_single_rank("SIMPLE_RADIAL", False, 2, "split", mp),
    "sharded_w3_split": lambda mp: TD.test_sharded_equals_single_rank("SIMPLE_PINHOLE", False, 3, "split", mp),
    # projection / filter / cam_from_img with fp32 and fp64 tracks, radial distortion
    **{f"geom_{name}_{dt}": (lambda mp, name=name, dt=dt: (dt == "f64" and _f64_tracks(mp, TG),
                                                          TG.test_project_and_cam_from_img_golden(GOLDEN, name),
                                                          TG.test_filter_golden_bit_exact(GOLDEN, name, 1, 4),
                                                          TG.test_filter_golden_bit_exact(GOLDEN, name, 0, 1)))
       for name in ("radial", "opencv4") for dt in ("f32", "f64")},
    # triangulation: several reference chunks in one launch; by pair
    "tri_s24_chunked": lambda mp: TT.test_triangulate_tracks_golden(GOLDEN, "s24_chunked"),
    "tri_s200_chunked": lambda mp: TT.test_triangulate_tracks_golden(GOLDEN, "s200_chunked"),
    "tri_by_pair": lambda mp: TT.test_triangulate_by_pair_golden(GOLDEN),
    # fundamental matrix: partial valid_mask, second_refine (estimate_fundamental's default); the two-view stage
    "fmat_seven_point_score": lambda mp: TF.test_seven_point_and_score_match_oracle_bitwise(),
    "fmat_estimate": lambda mp: TF.test_estimate_fundamental_matches_oracle(2, 700, 128, 24),
    "fmat_preliminary": lambda mp: TF.test_estimate_preliminary_cameras_on_a_scene(),
    # P3P RANSAC (plain and virtual focal frames) and pose refinement
    "p3p_plain": lambda mp: TP.test_p3p_ransac_matches_oracle_on_same_samples(5, 700, 256, 1),
    "p3p_groups": lambda mp: TP.test_p3p_ransac_matches_oracle_on_same_samples(6, 300, 64, 3),
    "pose_refine": lambda mp: TPO.test_pose_refinement_matches_oracle("SIMPLE_RADIAL", 3),
    # 5 inliers of 800: 251 of the block's 256 lanes add nothing, so the block reduction is all there is to get wrong
    "pose_refine_5_inliers": lambda mp: TPR.test_parity("n5_fk"),
    # dense depth: sparse depth, align, apply, unproject
    "dense_depth": lambda mp: (TDD.test_sparse_depth_matches_reference("radial_shared"),
                               TDD.test_align_replays_sklearn_draws("radial_shared"),
                               TDD.test_apply_and_unproject_bit_exact_with_reference_fit("radial_shared"),
                               TDD.test_align_dense_depth_maps_end_to_end("radial_shared")),
    # reprojection video: stats / visible / draw, the grids re-used across chunks (max_grid_cells=1), filter_mask
    "reproj_video": lambda mp: (TR.test_draw_list_and_stats_match_reference("center_r3"),
                                TR.test_frames_match_raster_restatement("center_r3"),
                                TR.test_chunked_grids_give_the_same_frames(),
                                TR.test_filter_invisible_reprojections_matches_reference()),
}


# read-backs that are not outputs: chol_envelope's #3 is its whole workspace (ws.cpu()), of which the test checks the tile map
# the device derived; the rest (T blocks, flags) is scratch
IGNORE = {"chol_envelope": {3}}


@pytest.mark.parametrize("name", list(CASES))
def test_entry_on_poisoned_memory(name):
    _check_poisoned(CASES[name], IGNORE.get(name, ()))


# --- reduce-buffer contracts -----------------------------------------------------------------------------------------------
def _split_problem(S=22, shared=True):
    """More than 16 cameras, separate tile launches, one tile batch: phase 12 (the split query) says OK.  22 cameras with
    shared intrinsics (n = 134): the parts' round-up at W = 683, 684 and 1024 is more than the padding 1024 / 2048 that
    buffers 4 and 6 used to be carved with."""
    sc = make_scene(S, 1500, "SIMPLE_RADIAL", shared_camera=shared, seed=17)
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=17)
    prob, _, _ = BA.compile_problem(D(pts0), D(ext0), D(K0), D(sc.tracks), D(sc.mask), D(extra0), shared, "SIMPLE_RADIAL")
    return prob


@pytest.mark.parametrize("pattern", [0xFF, 0x7F])
def test_reduce_buffer_1_upper_triangle_is_zero(pattern):
    """include/vggsfm_amd.h: reduce buffer 1 = S | rhs, n^2 + n doubles with the strict upper triangle all zero -- what makes
    an all-reduce of buffer 1 (instead of phases 4 / 5) correct.  On a poisoned workspace, after every phase 1 and after the
    whole iteration (factorisation in place included)."""
    sc = make_scene(40, 1500, "SIMPLE_RADIAL", shared_camera=True, seed=29)
    ext0, K0, extra0, pts0 = perturb_for_ba(sc, seed=29)
    opts = prepare_ba_options()
    with poisoned_allocations(pattern):
        prob, _, _ = BA.compile_problem(D(pts0), D(ext0), D(K0), D(sc.tracks), D(sc.mask), D(extra0), True, "SIMPLE_RADIAL")
        s = ShardedBA(prob, opts)
        n = 6 * 40 + 2
        assert s.bufs[1].numel() == n * n + n
        upper = torch.triu(torch.ones(n, n, dtype=torch.bool, device="cuda"), 1)
        s.begin()
        for it in range(3):
            for ph, where in ((0, None), (1, "phase 1"), (2, None), (3, "phase 3")):
                s._phase(ph)
                if where is None:
                    continue
                S = s.bufs[1][:n * n].view(n, n)
                bad = int(((S != 0) & upper).sum())
                assert bad == 0, f"iteration {it}, after {where}: {bad} non-zero elements in the strict upper triangle"
                assert torch.isfinite(s.bufs[1][n * n:]).all()


@pytest.mark.parametrize("S,shared", [(22, True), (24, False)])
@pytest.mark.parametrize("W", [2, 3, 513, 514, 683, 684, 1024])
def test_split_exchange_regions_fit_the_carve(W, S, shared, monkeypatch):
    """Phases 7..11 with W ranks: buffer 4 = [A: W ca | B: W cb] must end before buffer 5 starts, and buffer 6 =
    [A: W ca | B: W (cb + 1)] must fit its count (ca, cb from the counts of buffers 7 and 4); likewise the one-piece forms
    (W c in buffer 4, W (c + 1) in buffer 6).  The header allows W <= 1024."""
    monkeypatch.setattr(BA, "MERGED_TILE_MAX_OBS", 0)
    prob = _split_problem(S, shared)
    s = ShardedBA(prob, prepare_ba_options())
    L = _lib.lib()
    assert L.vgg_ba_phase(*s._abi, 12, _lib.stream_ptr()) == 0
    address, a = _lib.reduce_buffer(*s._abi, 7)
    M = s.bufs[4].numel()
    assert 0 < a < M and address == s.bufs[4].data_ptr()
    ca, cb, c = -(-a // W), -(-(M - a) // W), -(-M // W)
    room4 = (s.bufs[5].data_ptr() - s.bufs[4].data_ptr()) // 8
    assert W * (ca + cb) <= room4, (W, W * (ca + cb) - M, room4 - M)
    assert W * ca + W * (cb + 1) <= s.bufs[6].numel(), (W, W * (ca + cb + 1) - M, s.bufs[6].numel() - M)
    assert W * c <= room4 and W * (c + 1) <= s.bufs[6].numel()


def test_split_exchange_at_1024_ranks_stays_in_its_buffers(monkeypatch):
    """Rank 0 of 1024 through begin, phase 12 and phases 7..10 on a poisoned workspace: the zero tails phases 8 and 10 write up
    to W ca and W (ca + cb) stay inside buffer 4, so buffer 5 (the reduce-scatter output, written by the collective only)
    still holds the poison everywhere but at element ca + cb, where phase 10 puts the rank's gradient maximum."""
    monkeypatch.setattr(BA, "MERGED_TILE_MAX_OBS", 0)
    W = 1024
    with poisoned_allocations(0xFF):
        prob = _split_problem()
        s = ShardedBA(prob, prepare_ba_options(), rank=0, world_size=W, all_reduce=lambda t, op: None,
                      split_exchange="emulated")
        assert s._split
        ca, cb = s._mine_a.numel(), s._mine_b.numel() - 1
        s.begin()
        s._phase(0)
        for ph in (7, 8, 9, 10):
            s._phase(ph)
        torch.cuda.synchronize()
        b5 = s.bufs[5].cpu().numpy()
        b4 = s._padded_a.cpu().numpy(), s._padded_b.cpu().numpy()
    changed = np.nonzero(~equals_pattern(b5, 0xFF))[0]
    assert changed.tolist() == [ca + cb], changed[:16].tolist()
    assert np.isfinite(b5[ca + cb]) and b5[ca + cb] >= 0
    # the padded parts are fully written: payload + zero tail
    assert all(np.isfinite(x).all() for x in b4)
