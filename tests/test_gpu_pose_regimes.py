"""GPU parity of ``vgg_pose_refine`` (vggsfm_amd/csrc/pose.hip) with the oracle on every case of tests/pose_cases.py:
rejected and invalid steps, all six terminations, inlier counts around the wavefront and the block and below the number
of unknowns, P down to 0, four losses, every option the kernel reads, both track precisions, non-finite data -- through a
raw driver of the C entry that returns the state arrays as the kernel left them and the whole summary.

The bars are those of tests/test_gpu_pose.py (final cost 1e-9 relative, pose 1e-8, intrinsics rtol 1e-9 / atol 1e-10) and
the integer summary is compared for equality; tests/test_pose_cases.py shows, without a GPU, that the oracle itself stays
inside them on every case under a disturbance some hundred times what another summation order brings, so no case is left
out here.

NaN cost: both solvers report a problem whose cost is NaN (`nan_point`) as a GRADIENT exit after 0 iterations with the
state untouched, because `fmax` drops the NaN out of the gradient's max norm; Ceres itself would report a failure.
Nothing in the product reads `termination` of a pose refinement, so the two are left agreeing with each other.
"""
import struct

import numpy as np
import pytest
import torch

from oracle import ba as OB
from tests import pose_cases as PC
from vggsfm_amd import _lib
from vggsfm_amd.ba_options import AbsolutePoseRefinementOptions
from vggsfm_amd.pose import pose_refinement_batch

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in PC.CASES]


def _bits(x):
    return np.ascontiguousarray(x).tobytes()


def _summary_bits(s):
    return struct.pack("<2d5i", s["initial_cost"], s["final_cost"], *(s[k] for k in PC.INT_KEYS))


def _rel(a, b, tol):
    return a == b if b == 0 else abs(a - b) <= tol * abs(b)


def check_parity(name, q, t, intr, g):
    """The kernel's state (the whole arrays of the case's scene, as it left them) and summary `g` against the oracle."""
    case = PC.BY_NAME[name]
    pb, ext_o, intr_o, so = PC.solved(name)
    f, q_in, t_in, i_in = pb["frame"], pb["q0"], pb["t0"], pb["intr0"]
    print(f"{name}: kernel {[g[k] for k in PC.INT_KEYS]} cost {g['initial_cost']!r} -> {g['final_cost']!r}; "
          f"oracle {[so[k] for k in PC.INT_KEYS]} cost {so['initial_cost']!r} -> {so['final_cost']!r}")
    for k in PC.INT_KEYS:
        assert g[k] == so[k], (name, k, g, {k: so[k] for k in PC.INT_KEYS})
    # what the kernel was not asked to touch: every other row, the principal point, unrefined intrinsics
    others = np.arange(len(q)) != f
    assert _bits(q[others]) == _bits(q_in[others]) and _bits(t[others]) == _bits(t_in[others])
    assert _bits(intr[others]) == _bits(i_in[others])
    assert _bits(intr[f, 1:3]) == _bits(i_in[f, 1:3])
    if not case.flags & 1:
        assert _bits(intr[f, 0]) == _bits(i_in[f, 0])
    if not case.flags & 2 or case.model == "SIMPLE_PINHOLE":
        assert _bits(intr[f, 3]) == _bits(i_in[f, 3])
    if not case.finite:
        assert np.array_equal([g["initial_cost"], g["final_cost"]], [so["initial_cost"], so["final_cost"]], equal_nan=True)
        assert _bits(q[f]) == _bits(q_in[f]) and _bits(t[f]) == _bits(t_in[f]) and _bits(intr[f]) == _bits(i_in[f])
        assert np.isfinite(q).all() and np.isfinite(t).all() and np.isfinite(intr).all()
        return
    assert _rel(g["initial_cost"], so["initial_cost"], 1e-9), (g["initial_cost"], so["initial_cost"])
    if PC.is_exact_fit(so):
        assert g["final_cost"] < 1e-9 * so["initial_cost"], (g["final_cost"], so["final_cost"], so["initial_cost"])
    else:
        assert _rel(g["final_cost"], so["final_cost"], 1e-9), (g["final_cost"], so["final_cost"])
    q_o = OB.rotmat_to_quat(ext_o[:, :3])
    dq = min(np.abs(q[f] - q_o).max(), np.abs(q[f] + q_o).max())
    dt = np.abs(t[f] - ext_o[:, 3]).max()
    print(f"{name}: |dq| {dq:.2e} |dt| {dt:.2e} |dintr| {np.abs(intr[f] - intr_o).max():.2e}")
    assert dq <= 1e-8 and dt <= 1e-8, (dq, dt)
    np.testing.assert_allclose(np.concatenate([OB.quat_to_rotmat(q[f]), t[f][:, None]], -1), ext_o, atol=1e-8)
    np.testing.assert_allclose(intr[f], intr_o, rtol=1e-9, atol=1e-10)


@pytest.mark.parametrize("name", NAMES)
def test_parity(name):
    q, t, intr, sums = PC.run_case(name)
    assert len(sums) == 1 and sums[0]["frame"] == PC.solved(name)[0]["frame"]
    check_parity(name, q, t, intr, sums[0])


# --- batches ------------------------------------------------------------------------------------------------------------
def _group_key(name):
    pb = PC.solved(name)[0]
    return (pb["model"], pb["loss"], pb["scale"], bytes(pb["options"]), pb["tracks"].dtype.str, pb["points"].shape,
            _bits(pb["points"]))


def _groups():
    groups = {}
    for n in NAMES:
        groups.setdefault(_group_key(n), []).append(n)
    return sorted(groups.values(), key=lambda g: NAMES.index(g[0]))


GROUPS = _groups()


def _stack(names):
    """One launch for the cases of a group: row i + 1 (+ 1 past the middle) is the frame of case i, rows 0 and the middle
    one are frames nobody lists (copies of a neighbour's data: a kernel that strayed there would have something to solve)."""
    pbs = [PC.solved(n)[0] for n in names]
    rows, pick, spare = [], {}, [0, 1 + len(names) // 2]
    for i, (n, pb) in enumerate(zip(names, pbs)):
        while len(rows) in spare:
            rows.append((pb, pb["frame"]))
        pick[n] = len(rows)
        rows.append((pb, pb["frame"]))
    take = lambda key: np.ascontiguousarray(np.stack([pb[key][f] for pb, f in rows]))
    return pick, spare, {k: take(k) for k in ("q0", "t0", "intr0", "tracks", "mask", "flags")}, pbs[0]


@pytest.mark.parametrize("names", GROUPS, ids=[g[0] for g in GROUPS])
def test_batch_is_bit_identical_to_single_launches(names):
    """All cases that share points, model, loss, options and track precision in ONE launch, `frame_ids` shuffled and a
    proper subset of the rows, refine flags differing from row to row: every frame's state and summary bit-identical to
    its own launch, unlisted rows untouched, a second launch bit-identical to the first."""
    pick, spare, a, pb0 = _stack(names)
    order = [pick[n] for n in names]
    np.random.Generator(np.random.PCG64(len(names))).shuffle(order)
    assert set(order).isdisjoint(spare) and len(order) < len(a["q0"])
    if len(names) > 3:
        assert order != sorted(order)
    launch = lambda: PC.run_rows(a["q0"], a["t0"], a["intr0"], a["tracks"], pb0["points"], a["mask"], a["flags"], order,
                                 pb0["model"], pb0["options"], pb0["loss"], pb0["scale"])
    q, t, intr, sums = launch()
    q2, t2, intr2, sums2 = launch()
    assert _bits(q) == _bits(q2) and _bits(t) == _bits(t2) and _bits(intr) == _bits(intr2)
    assert [_summary_bits(s) for s in sums] == [_summary_bits(s) for s in sums2]
    assert [s["frame"] for s in sums] == order
    for r in spare:
        assert _bits(q[r]) == _bits(a["q0"][r]) and _bits(t[r]) == _bits(a["t0"][r]) and _bits(intr[r]) == _bits(a["intr0"][r])
    by_row = {s["frame"]: s for s in sums}
    for n in names:
        qs, ts, is_, ss = PC.run_case(n)
        f, r = PC.solved(n)[0]["frame"], pick[n]
        assert _bits(q[r]) == _bits(qs[f]) and _bits(t[r]) == _bits(ts[f]) and _bits(intr[r]) == _bits(is_[f]), n
        assert _summary_bits(by_row[r]) == _summary_bits(ss[0]), (n, by_row[r], ss[0])


def test_groups_mix_flags_and_cover_the_table():
    assert sorted(n for g in GROUPS for n in g) == sorted(NAMES)
    big = max(GROUPS, key=len)
    assert len(big) >= 20 and {PC.BY_NAME[n].flags for n in big} == {0, 1, 2, 3}


# --- precisions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["easy_radial_fk", "hard_pinhole_f", "n5_fk", "n65_pose", "loss_huber_hard",
                                  "behind_radial_pose_hard", "inf_observation_f32"])
def test_widened_float32_tracks_are_bit_identical(name):
    """The kernel widens float32 tracks on load: the same values handed over as float64 give the same bits."""
    pb = PC.solved(name)[0]
    assert pb["tracks"].dtype == np.float32
    q, t, intr, sums = PC.run_case(name)
    q2, t2, intr2, sums2 = PC.run_rows(pb["q0"], pb["t0"], pb["intr0"], pb["tracks"].astype(np.float64), pb["points"],
                                       pb["mask"], pb["flags"], [pb["frame"]], pb["model"], pb["options"], pb["loss"],
                                       pb["scale"])
    assert _bits(q) == _bits(q2) and _bits(t) == _bits(t2) and _bits(intr) == _bits(intr2)
    assert _summary_bits(sums[0]) == _summary_bits(sums2[0])


# --- the entry's contract at P = 0 ---------------------------------------------------------------------------------------
def test_entry_rejects_null_pointers_and_accepts_P0():
    """include/vggsfm_amd.h: P >= 0, and NULL pointers are invalid arguments.  An empty torch tensor has a NULL data
    pointer, so a caller with P = 0 must hand over allocated buffers (PC.to_device does; `P0_*` of the table run that way)."""
    pb = PC.solved("P0_fk")[0]
    q, t, i = PC.to_device(pb["q0"]), PC.to_device(pb["t0"]), PC.to_device(pb["intr0"])
    args = (pb["mask"].shape[0], 0, [pb["frame"]], PC.to_device(pb["flags"]), pb["model"], pb["options"], 1, 1.0)
    one = torch.zeros(1, dtype=torch.float64, device="cuda")
    for tracks, points, mask in ((None, one, one), (one, None, one), (one, one, None)):
        rc, _ = PC.run_kernel(q, t, i, tracks, points, mask, *args, check=False)
        assert rc == -1                                              # VGG_ERR_INVALID_ARGUMENT
    assert _bits(q.cpu().numpy()) == _bits(pb["q0"]) and _bits(i.cpu().numpy()) == _bits(pb["intr0"])
    rc, sums = PC.run_kernel(q, t, i, one, one, one, *args, check=False)
    assert rc == _lib.VGG_OK and sums[0]["num_iterations"] == 0 and sums[0]["termination"] == 1
    assert sums[0]["initial_cost"] == 0.0 and sums[0]["final_cost"] == 0.0
    assert _bits(q.cpu().numpy()) == _bits(pb["q0"]) and _bits(t.cpu().numpy()) == _bits(pb["t0"])


# --- the product's wrapper -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["refopts_cap_3_cauchy_2", "refopts_gradient_cauchy_2"])
def test_wrapper_forwards_refinement_options(name):
    """`pose_refinement_batch` with non-default AbsolutePoseRefinementOptions -- the only way the product's callers set
    gradient_tolerance, max_num_iterations and loss_function_scale -- against the oracle under the same options."""
    case = PC.BY_NAME[name]
    pb, ext_o, intr_o, so = PC.solved(name)
    o = pb["options"]
    ref = AbsolutePoseRefinementOptions(gradient_tolerance=o.gradient_tolerance, max_num_iterations=o.max_num_iterations,
                                        loss_function_scale=case.scale)
    assert (ref.gradient_tolerance, ref.max_num_iterations, ref.loss_function_scale) != (1.0, 100, 1.0)
    f = pb["frame"]
    ext, prm, sums = pose_refinement_batch(PC.to_device(pb["ext0"]), PC.to_device(pb["intr0"]), PC.to_device(pb["tracks"]),
                                           PC.to_device(pb["points"]), torch.from_numpy(pb["mask"]).cuda(), [f], pb["model"],
                                           torch.from_numpy(pb["flags"]), ref)
    ext, prm = ext.cpu().numpy(), prm.cpu().numpy()
    g = sums[0]
    assert g["frame"] == f
    for k in PC.INT_KEYS:
        assert g[k] == so[k], (k, g, so[k])
    assert _rel(g["initial_cost"], so["initial_cost"], 1e-9) and _rel(g["final_cost"], so["final_cost"], 1e-9)
    np.testing.assert_allclose(ext[f], ext_o, atol=1e-8)
    np.testing.assert_allclose(prm[f], intr_o, rtol=1e-9, atol=1e-10)
    others = np.arange(len(ext)) != f
    assert _bits(ext[others]) == _bits(pb["ext0"][others]) and _bits(prm[others]) == _bits(pb["intr0"][others])
