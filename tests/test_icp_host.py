"""CPU tests of the registration library: what its C-ABI registry has of its own (the registry itself is
tests/test_side_libraries.py's), the one copy of the grid walk, what the entries refuse, and the yardstick of the GPU tests
(the all-pairs NumPy restatement of tests/icp_cases.py) against independent answers: torch-autograd's gradient and
Gauss-Newton matrix, scipy's k-d tree, recovery of a known transform, the analytic normals of the base scene; and the margins
of every decision the GPU tests compare exactly.  No kernel is called here."""
import os
import re

import numpy as np
import pytest

from tests import icp_cases as C
from tests.test_c_abi import _parse_header
from vggsfm_amd import _lib_icp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vggi_build_arch", "vggi_icp_step", "vggi_icp_step_mesh", "vggi_icp_sums", "vggi_icp_update", "vggi_radius_normals"]
GAP_FLOOR = 1e-9           # relative to r2; rounding differences would show at 1e-16
EIGEN_GAP_FLOOR = 0.05


# --------------------------------------------------------------------------------------------------- registry
def test_header_table_and_library_agree():
    """What only the registration has (tests/test_side_libraries.py compares table, header and symbols): the names and
    prototypes pinned by hand, the header's constants against the binding and the restatement, and the one grid walk."""
    header = open(_lib_icp.HEADER_PATH).read()
    functions, _ = _parse_header(header)
    assert list(_lib_icp.SIGNATURES) == list(functions) == NAMES
    grid = ["double"] * 4 + ["int"] * 3
    tail = ["pointer", "double", "double", "int", "int", "int", "double", "pointer", "pointer", "pointer"]
    assert functions["vggi_icp_step"] == ("int", ["pointer", "pointer", "int", "pointer", "pointer", "pointer", "int"] + grid + ["pointer"] + tail)
    assert functions["vggi_icp_step_mesh"][1] == ["pointer", "pointer", "int", "pointer", "int", "pointer", "int", "pointer", "pointer",
                                                  "int"] + grid + tail
    assert functions["vggi_icp_update"][1] == ["pointer", "pointer", "int", "int"] + ["double"] * 4 + ["pointer", "int", "pointer"]
    assert functions["vggi_radius_normals"][1] == ["pointer"] * 3 + ["int"] + grid + ["double", "double", "int"] + ["pointer"] * 5
    consts = dict(re.findall(r"#define VGGI_(\w+) ([\de.-]+)", header))
    assert {k: int(consts[k]) for k in ("GROUPS", "BLOCK", "WORDS", "STATE_WORDS", "HISTORY_WORDS", "NORMAL_SWEEPS")} == \
        dict(GROUPS=_lib_icp.GROUPS, BLOCK=_lib_icp.BLOCK, WORDS=_lib_icp.WORDS, STATE_WORDS=_lib_icp.STATE_WORDS,
             HISTORY_WORDS=_lib_icp.HISTORY_WORDS, NORMAL_SWEEPS=_lib_icp.NORMAL_SWEEPS)
    assert float(consts["PIVOT_MIN"]) == _lib_icp.PIVOT_MIN == C.PIVOT_MIN
    assert (C.GROUPS, C.BLOCK, C.WORDS) == (_lib_icp.GROUPS, _lib_icp.BLOCK, _lib_icp.WORDS)
    assert [int(consts[k]) for k in ("RUNNING", "CONVERGED", "TOO_FEW", "DEGENERATE")] == [0, 1, 2, 3]
    assert _lib_icp.STATUS == C.STATUS == ("running", "converged", "too few", "degenerate")
    # one copy of the grid walk: the helpers stand in nn_grid.hpp and in neither .hip file
    nn = open(os.path.join(ROOT, "vggsfm_amd", "csrc", "nn", "nn.hip")).read()
    icp = open(os.path.join(ROOT, "vggsfm_amd", "csrc", "icp", "icp.hip")).read()
    shared = open(os.path.join(ROOT, "vggsfm_amd", "csrc", "nn", "nn_grid.hpp")).read()
    for helper in ("struct Grid", "bool finite3(", "int axis_cell(", "void axis_range(", "double dot3(", "struct Triangle",
                   "bool face_vertices(", "void closest_point("):
        assert shared.count(helper) == 1 and helper not in nn and helper not in icp, helper
    assert '#include "nn_grid.hpp"' in nn and '#include "../nn/nn_grid.hpp"' in icp


# --------------------------------------------------------------------------------------------------- refusals
def test_host_refusals_need_no_device():
    """What the entries refuse is decided on the host, before any launch (NULL pointers throughout)."""
    import ctypes

    L = _lib_icp.lib()
    nan = float("nan")
    good = dict(m=4, n=5, V=6, F=3, P=7, cell=0.5, dims=(5, 3, 2), r=0.4, r2=0.16, metric=0, loss=0, k=0.0)
    one = ctypes.c_void_p(8)               # a non-NULL pointer that is never dereferenced: every call below is refused

    def grid(a):
        return (0.0, 0.0, 0.0, a["cell"], *a["dims"])

    def step(normals=None, **kw):
        a = dict(good, **kw)
        return L.vggi_icp_step(None, None, a["m"], None, None, None, a["n"], *grid(a), normals, None, a["r"], a["r2"], a["metric"], 1,
                               a["loss"], a["k"], None, None, None)

    def mesh(**kw):
        a = dict(good, **kw)
        return L.vggi_icp_step_mesh(None, None, a["m"], None, a["V"], None, a["F"], None, None, a["P"], *grid(a), None, a["r"], a["r2"],
                                    a["metric"], 1, a["loss"], a["k"], None, None, None)
    bad_grid = (dict(cell=0.0), dict(cell=-1.0), dict(cell=nan), dict(dims=(0, 3, 2)), dict(dims=(5, -1, 2)), dict(dims=(5, 3, 0)),
                dict(dims=(2 ** 13, 2 ** 12, 2)), dict(dims=(2 ** 25 + 1, 1, 1)))
    bad = bad_grid + (dict(r=0.0), dict(r=-1.0), dict(r=nan), dict(r2=nan), dict(r2=-1.0), dict(m=-1), dict(metric=2), dict(metric=-1),
                      dict(loss=3), dict(loss=-1), dict(loss=1, k=0.0), dict(loss=2, k=nan), dict(loss=1, k=-1.0))
    for entry, more in ((step, (dict(n=-1),)), (mesh, (dict(V=-1), dict(F=-1), dict(P=-1)))):
        assert entry() == -1 and entry(m=0) == -1, entry.__name__               # state and workspace are always needed
        for b in bad + more:
            assert entry(**dict(dict(m=0), **b)) == -1, (entry.__name__, b)
    assert step(metric=1) == -1 and step(metric=1, normals=one) == -1           # point to plane without normals; then no state
    assert L.vggi_icp_sums(None, None, None) == -1 and L.vggi_icp_sums(one, None, None) == -1 and L.vggi_icp_sums(None, one, None) == -1

    def update(ws=one, state=one, min_c=6, damping=0.0, tols=(0.0, 0.0, 0.0), history=None, rows=0):
        return L.vggi_icp_update(ws, state, 1, min_c, damping, *tols, history, rows, None)
    for kw in (dict(ws=None), dict(state=None), dict(min_c=0), dict(min_c=-3), dict(damping=-1.0), dict(damping=nan),
               dict(tols=(nan, 0.0, 0.0)), dict(tols=(0.0, nan, 0.0)), dict(tols=(0.0, 0.0, nan)), dict(rows=-1), dict(rows=3)):
        assert update(**kw) == -1, kw

    def normals(toward=None, **kw):
        a = dict(dict(good, mn=5), **kw)
        return L.vggi_radius_normals(None, None, None, a["n"], *grid(a), a["r"], a["r2"], a["mn"], toward, None, None, None, None)
    assert normals() == -1 and normals(n=0) == 0
    for b in bad_grid + (dict(r=0.0), dict(r=nan), dict(r2=-1.0), dict(n=-1), dict(mn=0)):
        assert normals(**dict(dict(n=0), **b)) == -1, b
    assert normals((ctypes.c_double * 3)(0.0, nan, 0.0), n=0) == -1 and normals((ctypes.c_double * 3)(0.0, 1.0, 2.0), n=0) == 0

    import torch
    from vggsfm_amd import registration
    p = torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        registration.make_target(p, 0.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        registration.estimate_normals(p, 0.5)
    fake = registration.Target(type("G", (), {"device": "cpu"})(), None, 0.5)
    with pytest.raises(ValueError, match="metric must be"):
        registration._options(fake, "plane", None, None)
    with pytest.raises(ValueError, match="loss must be"):
        registration._options(fake, "point_to_point", "cauchy", 1.0)
    with pytest.raises(ValueError, match="needs loss_scale > 0"):
        registration._options(fake, "point_to_point", "huber", None)
    assert registration._options(fake, "point_to_point", "tukey", 0.5) == (0, 2, 0.5)
    with pytest.raises(ValueError, match="must be finite"):
        registration.make_state(nan, torch.eye(3), torch.zeros(3), [0.0] * 3, "cpu")
    s = registration.make_state(2.0, torch.eye(3), torch.tensor([1.0, 2.0, 3.0]), [4.0, 5.0, 6.0], "cpu")
    assert s.tolist() == [0.0, 0.0, 2.0, 1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0] and len(s) == _lib_icp.STATE_WORDS


# --------------------------------------------------------------------------------- the restatement against truth
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("estimate_scale", [False, True])
@pytest.mark.parametrize("loss,k", [(0, 0.0), (1, 0.004), (2, 0.012)])
def test_normal_equations_are_autograds(metric, estimate_scale, loss, k):
    """With the pairs frozen, g is the gradient at 0 of 1/2 sum rho(|r(delta)|) and H the Gauss-Newton matrix
    sum w J^T J of the autograd Jacobians of the residuals, where x(delta) = c + (1 + lambda) Exp(omega) (x - c) + tau."""
    import torch

    c = C.step_cases()[f"metric{metric}_scale{int(estimate_scale)}_loss{loss}"]
    S = C.step(c["source"], c["target"], c["T"], c["center"], c["max_dist"], metric, estimate_scale, loss, k)
    keep = S["index"] >= 0
    x = torch.from_numpy(C.apply(c["T"], c["source"])[keep])
    y = torch.from_numpy(c["target"]["points"][S["index"][keep]])
    n = torch.from_numpy(c["target"]["normals"][S["index"][keep]])
    ctr = torch.tensor(c["center"], dtype=torch.float64)

    def residuals(delta):
        om, tau, lam = delta[:3], delta[3:6], delta[6] if estimate_scale else 0.0
        K = torch.zeros(3, 3, dtype=torch.float64)
        K[0, 1], K[0, 2], K[1, 0], K[1, 2], K[2, 0], K[2, 1] = -om[2], om[1], om[2], -om[0], -om[1], om[0]
        moved = ctr + (1.0 + lam) * ((x - ctr) @ torch.linalg.matrix_exp(K).T) + tau
        e = moved - y
        return (e * n).sum(1, keepdim=True) if metric == 1 else e

    def rho(s):                                        # of the residual norm s
        if loss == 1:
            return torch.where(s <= k, s * s, 2.0 * k * s - k * k)
        if loss == 2:
            q = torch.clamp(s / k, max=1.0)
            return (k * k / 3.0) * (1.0 - (1.0 - q * q) ** 3)
        return s * s

    zero = torch.zeros(7, dtype=torch.float64, requires_grad=True)
    total = 0.5 * rho(residuals(zero).norm(dim=1)).sum()
    (grad,) = torch.autograd.grad(total, zero)
    J = torch.autograd.functional.jacobian(lambda d: residuals(d).reshape(-1), torch.zeros(7, dtype=torch.float64))
    rows = J.shape[0] // int(keep.sum())
    w = torch.from_numpy(np.asarray(S["weights"], np.float64)).repeat_interleave(rows)
    H = (J * w[:, None]).T @ J
    scale = np.abs(S["abs_g"]).max()
    assert np.abs(grad.numpy() - S["g"]).max() <= 1e-12 * scale, (grad.numpy(), S["g"])
    assert np.abs(H.numpy() - S["H"]).max() <= 1e-12 * np.abs(S["H"]).max()
    if not estimate_scale:
        assert not S["H"][6].any() and not S["H"][:, 6].any() and S["g"][6] == 0.0
    w = np.asarray(S["weights"])
    if loss == 1:                                      # the loss bites on some pairs, not on all
        assert 0 < (w < 1).sum() < len(w) and (w > 0).all()
    elif loss == 2:
        assert 0 < (w == 0).sum() < len(w) and (w < 1).all()


@pytest.mark.parametrize("name", ["m1500", "nonfinite", "metric0_scale1_loss0"])
def test_pairs_match_the_kd_tree(name):
    from scipy.spatial import cKDTree

    c, ref = C.step_cases()[name], C.step_reference(name)
    pts = c["target"]["points"]
    ok = np.isfinite(pts).all(1)
    rows = np.nonzero(ok)[0]
    x = C.apply(c["T"], c["source"])
    fq = np.isfinite(x).all(1)
    d, i = cKDTree(pts[ok]).query(x[fq], k=1, distance_upper_bound=c["max_dist"])
    want = np.where(np.isfinite(d), rows[np.minimum(i, len(rows) - 1)], -1)
    normals = c["target"].get("normals")
    if normals is not None:
        want = np.where((want >= 0) & ~np.isfinite(normals[np.maximum(want, 0)]).all(1), -1, want)
    assert np.array_equal(ref["index"][fq], want) and (ref["index"][~fq] == -1).all() and ref["count"] == (want >= 0).sum()


@pytest.mark.parametrize("name", list(C.trajectory_cases()))
def test_restatement_recovers_the_known_transform(name):
    c = C.trajectory_cases()[name]
    for extended in (False, True):
        r = C.trajectory_reference(name, extended)
        err = C.transform_error(r["T"], c["truth"])
        print(f"\n{name} ({'long double' if extended else 'float64'}): {r['status']} after {r['iterations']}, error {err:.2e}, "
              f"cost {float(r['history'][-1][2]):.1e}")
        assert r["status"] == "converged" and r["iterations"] <= 5 and err <= 1e-12
    a, b = C.trajectory_reference(name), C.trajectory_reference(name, True)
    assert [h[0] for h in a["history"]] == [h[0] for h in b["history"]] and a["iterations"] == b["iterations"]
    yard = max(C.transform_error(p, q) for p, q in zip(a["transforms"], b["transforms"]))
    print(f"{name}: float64 against long double over the iterations: {yard:.2e}")
    assert 0.0 < yard < 1e-12


def test_normals_are_the_surfaces():
    _, analytic, _ = C.base_scene()
    ref = C.normals_reference("surface")
    toward = C.normals_reference("toward")                               # a viewpoint above: the normals of a graph point up
    angle = np.degrees(np.arccos(np.clip((toward["normal"] * analytic).sum(1), -1.0, 1.0)))
    print(f"\nPCA normals at radius {C.NORMAL_RADIUS}: within {angle.max():.2f} degrees of the analytic ones; smallest eigen-gap "
          f"{np.nanmin(ref['eigen_gap']):.3f}")
    assert angle.max() < 3.0 and (toward["normal"][:, 2] > 0).all()
    # without a viewpoint the first non-zero component is positive: the same line, one side or the other
    first = ref["normal"][:, 0]
    assert (first > 0).all() and np.array_equal(np.abs(ref["normal"]), np.abs(toward["normal"])) and (ref["normal"][:, 2] < 0).any()
    lonely = C.normals_reference("lonely")
    assert lonely["count"][-2:].tolist() == [2, 2] and np.isnan(lonely["normal"][-2:]).all()
    bad = C.normals_reference("nonfinite")
    assert bad["count"][[3, 77]].tolist() == [0, 0] and np.isnan(bad["normal"][[3, 77]]).all()


# --------------------------------------------------------------------------------------------- margins
def test_no_decision_of_a_gpu_case_is_a_tie():
    """The GPU tests compare the pairs exactly: over every step case and every iteration of every trajectory case the
    smallest (second - best) / r2 and |d2 - r2| / r2 stay above GAP_FLOOR, and the smallest eigen-gap of every normals case
    above EIGEN_GAP_FLOOR."""
    worst = [np.inf, np.inf]
    for name in C.step_cases():
        ref = C.step_reference(name)
        assert ref["gap_best"] > GAP_FLOOR and ref["gap_r2"] > GAP_FLOOR, name
        worst = [min(worst[0], ref["gap_best"]), min(worst[1], ref["gap_r2"])]
    for name in C.trajectory_cases():
        for extended in (False, True):
            ref = C.trajectory_reference(name, extended)
            assert ref["gap_best"] > GAP_FLOOR and ref["gap_r2"] > GAP_FLOOR, name
            worst = [min(worst[0], ref["gap_best"]), min(worst[1], ref["gap_r2"])]
    gaps = {name: float(np.nanmin(C.normals_reference(name)["eigen_gap"])) for name in C.normals_cases()}
    print(f"\nsmallest gaps: best/second {worst[0]:.3e}, d2/r2 {worst[1]:.3e} (floor {GAP_FLOOR:.0e}); eigen-gaps {gaps}")
    assert min(gaps.values()) > EIGEN_GAP_FLOOR
    assert min(C.normals_reference(name)["gap_r2"] for name in C.normals_cases()) > GAP_FLOOR
