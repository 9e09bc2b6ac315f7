"""The ICP kernels (csrc/icp/icp.hip) against the all-pairs NumPy restatement of tests/icp_cases.py: per step case the pairs
and their count BIT FOR BIT and every sum within the bound that holds for any order of summation; the same bits twice and
after calls on other data; the update against a long-double solve of the read-back system; the statuses; whole trajectories
against the restatement within a yardstick measured on the CPU; recovery of a known Sim(3); the radius normals."""
import numpy as np
import pytest
import torch

from tests import icp_cases as C

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
METRIC = {0: "point_to_point", 1: "point_to_plane"}
LOSS = {0: None, 1: "huber", 2: "tukey"}


def D(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _target(c):
    from vggsfm_amd import nearest, registration

    t = c["target"]
    if "faces" in t:
        return registration.Target(nearest.TriangleGrid(D(t["vertices"]), D(t["faces"]), c["cell"]), None, c["cell"])
    normals = None if t.get("normals") is None else D(t["normals"])
    return registration.Target(nearest.PointGrid(D(t["points"]), c["cell"]), normals, c["cell"])


def _transform(T):
    return float(T[0]), torch.from_numpy(np.asarray(T[1], np.float64)), torch.from_numpy(np.asarray(T[2], np.float64))


def _step(c, target=None, **kw):
    from vggsfm_amd import registration

    return registration.icp_step(D(c["source"]), _target(c) if target is None else target, _transform(c["T"]), c["max_dist"],
                                 METRIC[c["metric"]], c["estimate_scale"], LOSS[c["loss"]], c["loss_scale"] or None, c["center"],
                                 return_index=True, **kw)


def _flat(step):
    return np.concatenate([step.H.numpy().reshape(-1), step.g.numpy(), [step.cost, step.weight, step.sq_error, step.count]])


def _check_sums(name, got, ref, ext):
    """every sum within (count + 32) 2^-53 sum|terms| of the long-double restatement: the bound of ANY order of `count`
    additions (one rounding each), with 32 for the few roundings inside a term"""
    bound = (ext["count"] + 32) * U
    worst = 0.0
    for mine, exact, mass in ((got.H.numpy(), ext["H"], ext["abs_H"]), (got.g.numpy(), ext["g"], ext["abs_g"]),
                              (got.weight, ext["sum_w"], ext["abs_w"]), (got.cost, ext["sum_wr2"], ext["abs_wr2"]),
                              (got.sq_error, ext["sum_r2"], ext["abs_r2"])):
        err = np.abs(np.asarray(mine, np.longdouble) - exact)
        lim = bound * np.asarray(mass, np.longdouble)
        assert (err <= lim).all(), (name, np.asarray(err, np.float64), np.asarray(lim, np.float64))
        with np.errstate(all="ignore"):
            worst = max(worst, float(np.nanmax(np.where(lim > 0, err / np.where(lim > 0, lim, 1), 0.0))))
    return worst


@pytest.mark.parametrize("name", list(C.step_cases()))
def test_step_matches_restatement(name):
    c, ref, ext = C.step_cases()[name], C.step_reference(name), C.step_reference(name, True)
    got = _step(c)
    index = got.index.cpu().numpy()
    assert index.dtype == np.int32 and index.tobytes() == ref["index"].tobytes(), (name, np.nonzero(index != ref["index"])[0][:5])
    assert got.count == ref["count"] == ext["count"] == int((index >= 0).sum())
    worst = _check_sums(name, got, ref, ext)
    print(f"\n{name}: {got.count} pairs of {len(c['source'])}; worst error / bound {worst:.3f}; gaps {ref['gap_best']:.2e} {ref['gap_r2']:.2e}")
    H = got.H.numpy()
    assert np.array_equal(H, H.T)
    if not c["estimate_scale"]:
        assert not H[6].any() and got.g[6] == 0.0
    if got.count == 0:
        assert not H.any() and not got.g.numpy().any() and got.cost == got.weight == got.sq_error == 0.0


def test_same_bits_twice_after_other_data_and_bounded_under_another_visit_order():
    c = C.step_cases()["m1500"]
    target = _target(c)
    first = _step(c, target)
    other = C.step_cases()["mesh_sphere"]
    _step(other)
    _step(C.step_cases()["metric0_scale1_loss2"])
    again = _step(c, target)
    assert _flat(first).tobytes() == _flat(again).tobytes() and torch.equal(first.index, again.index)
    given = _step(c, target, visit=torch.arange(len(c["source"]), dtype=torch.int32))
    assert torch.equal(first.index, given.index) and given.count == first.count
    _check_sums("m1500, given order", given, None, C.step_reference("m1500", True))


def _solve_extended(H, g, n):
    """the long-double solve of H delta = -g over the first n unknowns, by Gaussian elimination with pivoting"""
    A = np.concatenate([np.asarray(H[:n, :n], np.longdouble), -np.asarray(g[:n], np.longdouble)[:, None]], 1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(A[k:, k])))
        A[[k, p]] = A[[p, k]]
        A[k] = A[k] / A[k, k]
        for i in range(n):
            if i != k:
                A[i] = A[i] - A[i, k] * A[k]
    return A[:, n]


@pytest.mark.parametrize("name", ["metric1_scale1_loss0", "metric1_scale0_loss1", "metric0_scale1_loss2", "mesh_plane_metric0"])
def test_update_solves_the_read_back_system(name):
    """one (step, update) on the device.  The DEVICE's increment is recovered from the state it composed -- lambda = s'/s - 1,
    omega from Exp(omega) = R' R^T (vee of the skew part times theta / sin theta), tau = t' - c - (1 + lambda) Exp(omega)(t - c)
    -- and equals the long-double solve of the read-back H, g within 64 kappa(H) 2^-53 |delta| (a backward-stable solve of the
    Jacobi-scaled system loses at most a small multiple of kappa u) plus 16 2^-53 x the size of the numbers the recovery
    subtracts; so do |omega|, |tau| and lambda of the history row, and the restatement's own increment; R stays orthogonal
    to 1e-15"""
    from vggsfm_amd import _lib_icp as I
    from vggsfm_amd import nearest, registration

    c = C.step_cases()[name]
    target, src = _target(c), D(c["source"])
    got = _step(c, target)
    state = registration.make_state(*_transform(c["T"]), c["center"], src.device)
    work = registration._workspace(src.device)
    r, r2 = nearest._radius(c["max_dist"])
    visit = registration._visit(target, src, state)
    registration._launch_step(src, visit, target, state, r, r2, c["metric"], c["estimate_scale"], c["loss"], c["loss_scale"], work, None)
    hist = torch.zeros(1, I.HISTORY_WORDS, dtype=torch.float64, device=src.device)
    registration.check(registration._L.vggi_icp_update(work, state, int(c["estimate_scale"]), 6, 0.0, 0.0, 0.0, 0.0, hist, 1,
                                                       registration.stream_ptr()), "vggi_icp_update")
    state, hist = state.cpu().numpy(), hist.cpu().numpy()[0]
    assert state[0] == 0.0 and state[1] == 1.0 and hist[0] == got.count
    assert hist[1:4].tolist() == [got.weight, got.cost, got.sq_error]
    n = 7 if c["estimate_scale"] else 6
    H, g = got.H.numpy(), got.g.numpy()
    delta = _solve_extended(H, g, n)
    d = 1.0 / np.sqrt(np.diag(H)[:n])
    kappa = np.linalg.cond((H[:n, :n] * d[:, None]) * d[None])
    S = dict(H=H, g=g, count=got.count)
    status, T1, norms, mine = C.update(S, c["T"], c["center"], c["estimate_scale"])
    assert status == 0
    lim = 64.0 * kappa * U * float(np.abs(delta).max())
    scaled = np.abs(np.asarray(mine[:n], np.longdouble) - delta).max()
    assert scaled <= lim
    # the device's own increment, out of the state before and after
    s0, R0, t0 = float(c["T"][0]), np.asarray(c["T"][1], np.float64), np.asarray(c["T"][2], np.float64)
    ctr = np.asarray(c["center"], np.float64)
    s1, R1, t1 = state[2], state[3:12].reshape(3, 3), state[12:15]
    E = R1 @ R0.T
    vee = 0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
    sin_th = np.linalg.norm(vee)
    omega = vee * (np.arcsin(sin_th) / sin_th if sin_th > 0 else 1.0)
    lam = s1 / s0 - 1.0
    tau = t1 - ctr - (1.0 + lam) * (E @ (t0 - ctr))
    device = np.concatenate([omega, tau, [lam]])[:n]
    size = 1.0 + float(np.abs(ctr).max()) + float(np.abs(t1).max()) + float(np.abs(t0).max())
    off = float(np.abs(np.asarray(device, np.longdouble) - delta).max())
    print(f"\n{name}: kappa {kappa:.2e}, |delta| {float(np.abs(delta).max()):.3e}; device - long double {off:.2e} (limit {lim:.2e} + "
          f"{16 * U * size:.2e}), restatement - long double {float(scaled):.2e}")
    assert off <= lim + 16.0 * U * size
    if c["estimate_scale"]:
        assert abs(hist[6] - float(delta[6])) <= lim
    assert abs(hist[4] - float(np.sqrt((delta[:3] ** 2).sum()))) <= 2 * lim and abs(hist[5] - float(np.sqrt((delta[3:6] ** 2).sum()))) <= 2 * lim
    R = state[3:12].reshape(3, 3)
    assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-15
    assert C.transform_error((state[2], R, state[12:15]), T1) <= 4 * lim * (1.0 + float(np.abs(ctr).max()) + float(np.abs(T1[2]).max()))


def test_statuses_and_later_launches_leave_the_state_alone():
    from vggsfm_amd import registration

    g = np.random.default_rng(3)
    xy = g.uniform(-1.0, 1.0, (900, 2))
    plane = np.concatenate([xy, np.zeros((900, 1))], 1)
    normals = np.tile([0.0, 0.0, 1.0], (900, 1))
    target = registration.Target(_target(dict(target=dict(points=plane, normals=normals), cell=0.2)).grid, D(normals), 0.2)
    src = D(plane[:400] + [0.01, 0.0, 0.02])
    reg = registration.icp(src, target, 0.2, iterations=5)
    assert reg.status == "degenerate" and reg.iterations == 0 and reg.history == []
    assert reg.scale == 1.0 and torch.equal(reg.R, torch.eye(3, dtype=torch.float64)) and not reg.t.any()      # untouched by 5 x 2 launches
    assert reg.fitness == 1.0 and abs(reg.rmse - 0.02) < 1e-12
    few = registration.icp(src[:5], target, 0.2, iterations=5, metric="point_to_point", min_correspondences=6)
    assert few.status == "too few" and few.iterations == 0 and few.scale == 1.0 and not few.t.any()
    ok = registration.icp(src[:5], target, 0.2, iterations=3, metric="point_to_point", min_correspondences=5)
    assert ok.status in ("running", "converged") and ok.iterations >= 1
    none = registration.icp(src + torch.tensor([0.0, 0.0, 9.0], dtype=torch.float64, device=src.device), target, 0.2, iterations=2)
    assert none.status == "too few" and none.fitness == 0.0 and np.isnan(none.rmse)
    empty = registration.icp(src[:0], target, 0.2, iterations=2)
    assert empty.status == "too few" and empty.fitness == 0.0


@pytest.mark.parametrize("name", list(C.trajectory_cases()))
def test_trajectory_follows_the_restatement_and_recovers_the_truth(name):
    """per iteration the counts are equal and the transform is within 16 x the yardstick of the restatement's: the largest
    float64-versus-long-double difference of the restatement over the iterations of this case (the factor covers the
    differing sum orders compounded over the iterations); the end is within 1e-12 of the truth"""
    from vggsfm_amd import registration

    c, ref, ext = C.trajectory_cases()[name], C.trajectory_reference(name), C.trajectory_reference(name, True)
    yard = max(C.transform_error(a, b) for a, b in zip(ref["transforms"], ext["transforms"]))
    t = c["target"]
    target = registration.make_target(_cloud(t["points"], t["normals"]), c["cell"])
    got = []
    for k in range(1, ref["iterations"] + 1):          # the transform after k iterations: k (step, update) pairs from the start
        reg = registration.icp(D(c["source"]), target, c["max_dist"], iterations=k, metric=METRIC[c["metric"]],
                               estimate_scale=c["estimate_scale"], center=c["center"])
        got.append(reg)
    final = got[-1]
    assert final.status == ref["status"] == "converged" and final.iterations == ref["iterations"]
    assert [h["count"] for h in final.history] == [h[0] for h in ref["history"]]
    worst = 0.0
    for k, (reg, T) in enumerate(zip(got, ref["transforms"])):
        err = C.transform_error((reg.scale, reg.R.numpy(), reg.t.numpy()), T)
        worst = max(worst, err)
        assert err <= 16.0 * yard, (name, k, err, yard)
    truth = C.transform_error((final.scale, final.R.numpy(), final.t.numpy()), c["truth"])
    print(f"\n{name}: {final.iterations} iterations; yardstick {yard:.2e}, worst difference to the restatement {worst:.2e}; "
          f"to the truth {truth:.2e}; rmse {final.rmse:.2e}, fitness {final.fitness}")
    assert truth <= 1e-12 and final.fitness == 1.0 and final.rmse < 1e-12
    again = registration.icp(D(c["source"]), target, c["max_dist"], iterations=ref["iterations"], metric=METRIC[c["metric"]],
                             estimate_scale=c["estimate_scale"], center=c["center"])
    assert again.scale == final.scale and torch.equal(again.R, final.R) and torch.equal(again.t, final.t) and again.history == final.history


def _cloud(points, normals):
    from vggsfm_amd import fusion

    n = len(points)
    return fusion.FusedCloud(D(points), D(normals), None, D(np.zeros(n, np.int32)), D(np.zeros(n, np.int32)), D(np.zeros((n, 2), np.int32)))


def test_stages_resort_and_robust_loss_reach_the_truth():
    from vggsfm_amd import registration

    c = C.trajectory_cases()["plane_scale"]
    t = c["target"]
    src = c["source"].copy()
    src[::50] += [0.0, 0.0, 0.08]                        # 30 gross outliers
    reg = registration.icp(D(src), _cloud(t["points"], t["normals"]), [0.2, 0.15], iterations=12, estimate_scale=True, loss="tukey",
                           loss_scale=0.05, resort_every=2)
    err = C.transform_error((reg.scale, reg.R.numpy(), reg.t.numpy()), c["truth"])
    print(f"\ntwo stages, Tukey, 30 outliers: {reg.status} after {reg.iterations}, error {err:.2e}")
    assert reg.status == "converged" and err <= 1e-9 and {h["stage"] for h in reg.history} == {0, 1}


@pytest.mark.parametrize("name", list(C.normals_cases()))
def test_radius_normals_match_restatement(name):
    from vggsfm_amd import registration

    c, ref = C.normals_cases()[name], C.normals_reference(name)
    got = registration.estimate_normals(D(c["points"]), c["radius"], c["min_neighbors"], c["toward"])
    assert got.count.cpu().numpy().tobytes() == ref["count"].tobytes()
    n, k = got.normal.cpu().numpy(), got.curvature.cpu().numpy()
    has = ~np.isnan(ref["normal"]).any(1)
    assert np.array_equal(np.isnan(n).any(1), ~has) and np.array_equal(np.isnan(k), ~has)
    assert np.nanmin(ref["eigen_gap"]) > 0.05 and np.abs(np.linalg.norm(n[has], axis=1) - 1.0).max() <= 4 * U
    angle = np.arcsin(np.minimum(np.linalg.norm(np.cross(n[has], ref["normal"][has]), axis=1), 1.0))
    same_side = (n[has] * ref["normal"][has]).sum(1) > 0
    print(f"\n{name}: {has.sum()} normals, largest angle to the restatement {angle.max():.2e} rad, curvature off by "
          f"{np.abs(k[has] - ref['curvature'][has]).max():.2e}")
    assert same_side.all() and angle.max() <= 1e-9 and np.abs(k[has] - ref["curvature"][has]).max() <= 1e-12
