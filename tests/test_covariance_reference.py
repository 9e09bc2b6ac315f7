"""The bundle adjustment covariance, the part that needs no GPU: the long-double reference of tests/covariance_cases.py by its
two routes (dense inverse of the whole J^T J against the Schur route) and the float64 deviation that sets the GPU tests' bounds;
argument validation before any launch; the host mapping (camera order undone, column labels).

Agreement of the two routes: both are long-double evaluations of the same quantity, so they may differ by what long-double
rounding does to either -- the float64 deviation of the case scaled by the ratio of the unit roundoffs, 2^-11 (64-bit against
53-bit significands) -- and the bound is 100 x that, at least 1e-16.  The measured figures are in covariance_cases' docstring."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import ba_system_cases as SC
from tests import covariance_cases as CC
from vggsfm_amd import _lib
from vggsfm_amd import ba as BA



@pytest.mark.parametrize("name", CC.CASES)
def test_reference_routes_and_float64_deviation(name):
    R = CC.reference(name)
    ref, pb = R.ref, R.pb
    print(f"\n{name}: n = {pb.n_red}, {pb.P} points, {len(pb.obs_cam)} observations, reference in {R.seconds:.1f} s")
    for k in CC.BLOCKS:
        print(f"  float64 (B) against long double (B)  {k:16s} {R.dev[k]:9.2e}   GPU bound {R.bounds[k]:9.2e}")
    act = pb.active[:pb.n_red]
    d = np.diag(ref.reduced).astype(np.float64)
    assert (d[act] > 0).all() and (d[~act] == 0).all()
    assert (ref.reduced == ref.reduced.T).all() or np.abs((ref.reduced - ref.reduced.T).astype(np.float64)).max() <= 1e-17 * d.max()
    pt_act = pb.active[pb.n_red::3]
    vx = np.diagonal(ref.points, axis1=1, axis2=2).astype(np.float64)
    assert (vx[pt_act] > 0).all() and (ref.points[~pt_act] == 0).all()
    if name in CC.DENSE_CASES:
        dense = CC.dense_route(R.arrays, pb, R.blocks, CC.LD)
        for k, (err, zeros) in CC.errors(dense, ref).items():
            bound = max(1e-16, 100.0 * 2.0 ** -11 * R.dev[k])
            print(f"  (A) dense against (B) Schur, long double  {k:16s} {err:9.2e}   bound {bound:9.2e}")
            assert zeros and err <= bound, (k, err, bound)


def test_case_edges_reach_the_covariance():
    """What each case is in the table for, seen in the reference: zero blocks of constant poses, points and unobserved frames;
    a Cauchy case whose weights differ from 1; per-camera intrinsics blocks."""
    j = CC.reference("j")
    assert (j.ref.pose[:5] == 0).all() and (np.diagonal(j.ref.pose[5:], axis1=1, axis2=2) > 0).all()
    const = j.arrays.pt_const.astype(bool)
    assert const.sum() == 150 and (j.ref.points[const] == 0).all()
    # the constant points constrain the cameras: without their observations the reduced system is another one
    keep = ~const[j.pb.obs_pt]
    _, r, F, E, cols = j.blocks
    H_all = np.zeros((j.pb.n_red,) * 2)
    np.add.at(H_all, (cols[:, :, None], cols[:, None, :]), np.einsum("oki,okj->oij", F, F))
    H_var = np.zeros_like(H_all)
    np.add.at(H_var, (cols[keep][:, :, None], cols[keep][:, None, :]), np.einsum("oki,okj->oij", F[keep], F[keep]))
    assert np.abs(H_all - H_var).max() > 1e-3 * np.abs(H_all).max()
    g = CC.reference("g")
    assert (g.ref.pose[16:32] == 0).all() and (np.diagonal(g.ref.pose[32:], axis1=1, axis2=2) > 0).all()
    assert g.ref.intrinsics.shape == (1, 2, 2) and (np.diag(g.ref.intrinsics[0]) > 0).all()
    assert CC.reference("d").ref.intrinsics.shape == (33, 2, 2) and CC.reference("e").ref.intrinsics.shape == (33, 1, 1)
    assert CC.reference("i_none").ref.intrinsics.shape == (1, 0, 0)
    a = CC.reference("a")
    assert a.pb.n_red == 14 and (a.ref.pose[0] == 0).all() and a.ref.pose[1][3, 3] == 0 and a.ref.pose[1][4, 4] > 0


def test_cholesky_inverse_is_an_inverse():
    for n in (1, 14, 65):
        A, ref, dev, bound, res_bound = CC.spd_reference(n)
        assert np.abs((A.astype(CC.LD) @ ref - np.eye(n)).astype(np.float64)).max() < 1e-13
        assert dev < 1e-11 and bound >= SC.FLOOR_STEP
        assert (A == A.T).all() and np.linalg.cond(A) < 1e8


def _host_problem(name="a"):
    prob = SC.compile_case(name, "cpu")
    opt = SC.options_of(SC.CASES[name])
    prob.refine_focal, prob.refine_extra = opt.refine_focal_length, opt.refine_extra_params
    return prob, prob.c_struct(), BA._c_options(opt, overlap=False)


def test_entries_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    one = torch.zeros(64, dtype=torch.float64)          # (host memory: nothing is launched on these paths)
    flag = torch.zeros(1, dtype=torch.int32)
    bad, workspace, unsupported = -1, -3, -4
    assert L.vggc_spd_inverse_workspace_bytes(0) == 0 and L.vggc_spd_inverse_workspace_bytes(-3) == 0
    assert L.vggc_spd_inverse_workspace_bytes(10 ** 6) == 0
    n = 770
    need = L.vggc_spd_inverse_workspace_bytes(n)
    assert need >= 8 * (n * n + n) + 8 * 13 * 64 * 64 + L.vgg_cholesky_workspace_bytes(n) and need % 256 == 0
    assert L.vggc_spd_inverse(one, -1, one, flag, None) == bad
    assert L.vggc_spd_inverse(None, 0, None, None, None) == 0                               # nothing to invert: a no-op
    assert L.vggc_spd_inverse(None, 8, one, flag, None) == bad
    assert L.vggc_spd_inverse(one, 8, None, flag, None) == bad
    assert L.vggc_spd_inverse(one, 8, one, None, None) == bad
    assert L.vggc_spd_inverse(one, 10 ** 6, one, flag, None) == unsupported
    with pytest.raises(ctypes.ArgumentError):
        L.vggc_spd_inverse(one, 2 ** 31, one, flag, None)

    prob, cp, co = _host_problem()
    P, O = ctypes.byref(cp), ctypes.byref(co)
    need = L.vggc_ba_covariance_workspace_bytes(P, O, 3)
    assert need > L.vgg_ba_workspace_bytes(P, O) + 8 * 14 * 14 and need % 256 == 0
    assert L.vggc_ba_covariance_workspace_bytes(None, O, 3) == 0 and L.vggc_ba_covariance_workspace_bytes(P, None, 3) == 0
    outs = (one, one, one, one, one)
    assert L.vggc_ba_covariance(None, O, one, need, 3, *outs, flag, None) == bad
    assert L.vggc_ba_covariance(P, None, one, need, 3, *outs, flag, None) == bad
    assert L.vggc_ba_covariance(P, O, None, need, 3, *outs, flag, None) == bad
    assert L.vggc_ba_covariance(P, O, one, need, 3, *outs, None, None) == bad
    assert L.vggc_ba_covariance(P, O, one, need, 0, *outs, flag, None) == bad               # nothing selected
    assert L.vggc_ba_covariance(P, O, one, need, 4, *outs, flag, None) == bad               # an unknown flag
    assert L.vggc_ba_covariance(P, O, one, need, 2, one, one, one, one, None, flag, None) == bad   # points asked for, no room
    assert L.vggc_ba_covariance(P, O, one, need - 256, 3, *outs, flag, None) == workspace
    cp.camera_model = 5
    assert L.vggc_ba_covariance(P, O, one, need, 3, *outs, flag, None) == unsupported
    cp.camera_model, cp.num_intr = 0, 3
    assert L.vggc_ba_covariance(P, O, one, need, 3, *outs, flag, None) == unsupported
    cp.num_intr, cp.num_pts = 2, -1
    assert L.vggc_ba_covariance(P, O, one, need, 3, *outs, flag, None) == bad
    cp.num_pts, cp.num_cams, cp.num_intr = 1, 0, 0
    assert L.vggc_ba_covariance(P, O, None, 0, 1, None, None, None, None, None, None, None) == 0   # no cameras: a no-op
    cp.num_cams = cp.num_intr = 10 ** 4
    assert L.vggc_ba_covariance(P, O, one, need, 1, *outs, flag, None) == unsupported       # n beyond the index arithmetic
    # the additive reduce-buffer value: the scales' address and count, host code only
    prob, cp, co = _host_problem("c")
    fake = (ctypes.c_char * 64)()
    assert _lib.reduce_buffer(ctypes.byref(cp), ctypes.byref(co), fake, 8)[1] == 6 * 17 + 2
    assert L.vgg_ba_reduce_buffer(ctypes.byref(cp), ctypes.byref(co), fake, 9, ctypes.byref(ctypes.c_void_p()),
                                  ctypes.byref(ctypes.c_size_t())) == bad


# --- the host mapping ------------------------------------------------------------------------------------------------
def test_columns_and_frame_order_undo_the_camera_permutation():
    prob = SC.compile_case("l_env", "cpu")
    opt = SC.options_of(SC.CASES["l_env"])
    prob.refine_focal, prob.refine_extra = opt.refine_focal_length, opt.refine_extra_params
    perm = prob.cam_perm.tolist()
    S = len(perm)
    assert perm != list(range(S))
    cols = BA.covariance_columns(prob)
    assert len(cols) == 6 * S + 2 == 770
    for s in (0, 1, 2, S // 2, S - 1):
        assert cols[6 * s:6 * s + 6] == [("pose", perm[s], c) for c in BA.POSE_COMPONENTS]
    assert cols[6 * S:] == [("intrinsics", 0, "f"), ("intrinsics", 0, "k")]
    # a per-camera quantity of the problem lands at the frame it belongs to
    tag = torch.as_tensor(perm, dtype=torch.float64)[:, None, None].expand(S, 6, 6)
    back = BA.to_frame_order(prob, tag)
    assert (back[:, 0, 0] == torch.arange(S, dtype=torch.float64)).all()
    # per-camera intrinsics: labelled with their frame; no permutation: the identity
    d = SC.compile_case("d", "cpu")
    assert d.cam_perm is None and BA.to_frame_order(d, tag) is tag
    cd = BA.covariance_columns(d)
    assert cd[6 * 33:6 * 33 + 4] == [("intrinsics", 0, "f"), ("intrinsics", 0, "k"), ("intrinsics", 1, "f"), ("intrinsics", 1, "k")]
    e = SC.compile_case("e", "cpu")
    assert BA.covariance_columns(e)[6 * 33 + 5] == ("intrinsics", 5, "f") and len(BA.covariance_columns(e)) == 7 * 33
    n = SC.compile_case("i_none", "cpu")
    n.refine_focal = n.refine_extra = False
    assert len(BA.covariance_columns(n)) == 6 * 24


@pytest.mark.parametrize("name", CC.CASES)
def test_active_columns_are_the_references(name):
    """The host's count of active columns (num_active, the variance factor) uses the solver's rule, which is the reference's."""
    prob = SC.compile_case(name, "cpu")
    opt = SC.options_of(SC.CASES[name])
    prob.refine_focal, prob.refine_extra = opt.refine_focal_length, opt.refine_extra_params
    pb = CC.reference(name).pb
    mask = BA.active_columns(prob).numpy()
    assert mask.shape == (pb.n_red,) and (mask == pb.active[:pb.n_red]).all()


def test_public_surface():
    sig = inspect.signature(BA.estimate_covariance)
    assert [p.name for p in sig.parameters.values()] == ["problem", "options", "poses", "intrinsics", "points", "reduced"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("poses", "intrinsics", "points", "reduced"))
    assert [sig.parameters[k].default for k in ("poses", "intrinsics", "points", "reduced")] == [True, True, False, False]
    last = list(inspect.signature(BA.bundle_adjustment).parameters.values())[-1]
    assert last.name == "return_covariance" and last.default is False
    fields = [f.name for f in BA.BACovariance.__dataclass_fields__.values()]
    assert fields[:8] == ["pose", "intrinsics", "pose_intrinsics", "points", "reduced", "columns", "num_active", "variance_factor"]
    from vggsfm_amd import pycolmap_compat as PC
    assert list(inspect.signature(PC.estimate_ba_covariance).parameters) == ["reconstruction", "options", "config"]
    assert "pycolmap" in PC.estimate_ba_covariance.__doc__ and "cannot be read" in PC.estimate_ba_covariance.__doc__
