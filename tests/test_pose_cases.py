"""The pose-refinement case table (tests/pose_cases.py) judged on the CPU, from the oracle alone: every case is admitted
(the reference is stable on it, so the GPU suite has no reason to leave one out), the table as a whole covers the regimes
the device solver has, and the second derivation (oracle/ba_autograd.py) walks the same trajectory on every finite case."""
import numpy as np
import pytest

from oracle import ba as OB
from tests import pose_cases as PC
from tests.test_oracle_ba_second import _both, _compare

NAMES = [c.name for c in PC.CASES]


def _summaries():
    return {n: PC.solved(n)[3] for n in NAMES}


@pytest.mark.parametrize("name", NAMES)
def test_case_is_admitted(name):
    """Decisions clear of their thresholds by 1e-6, and five solves under a 1e-13 relative jitter of the points (about a
    thousand ulp) repeat the integer summary, the state to 1e-9 and the cost to 1e-9 relative (exact fits: stay below
    1e-9 of the initial cost; non-finite data: bit-identical)."""
    complaints = PC.admission(name)
    assert not complaints, complaints


def test_jitter_is_a_disturbance():
    """The admission's jitter does move the solve (a factor that rounded to 1 would admit anything)."""
    pb, ext, _, summ = PC.solved("hard_radial_fk")
    rng = np.random.Generator(np.random.PCG64(PC.JITTER_SEEDS[0]))
    pts = pb["points"] * (1.0 + PC.JITTER * rng.normal(size=pb["points"].shape))
    assert (pts != pb["points"]).mean() > 0.9
    e, _, s = PC.solve(PC.BY_NAME["hard_radial_fk"], pb, points=pts)
    assert e.tobytes() != ext.tobytes() and s["final_cost"] != summ["final_cost"]


def test_admission_rejects_the_known_unstable_problems():
    """The two regimes the oracle is chaotic on stay out, and the condition is what keeps them out."""
    far5 = PC.Case("far_frame5", model="SIMPLE_PINHOLE", flags=1, pert="far", frame=5)
    loose = PC.Case("no_tolerances", opt=PC._o(function_tolerance=0.0, gradient_tolerance=1e-12, parameter_tolerance=0.0))
    for c in (far5, loose):
        assert c.name not in PC.BY_NAME
        PC.BY_NAME[c.name] = c
        try:
            assert PC.admission(c.name), c.name
        finally:
            del PC.BY_NAME[c.name]
            PC.solved.cache_clear()


def test_table_covers_the_regimes():
    summ = _summaries()
    case = PC.BY_NAME
    # rejected steps: >= 4 cases with >= 3 each, both camera models, with and without intrinsics, one behind the camera
    rej = [n for n in NAMES if case[n].finite and summ[n]["num_unsuccessful_steps"] >= 3 and summ[n]["num_successful_steps"] >= 3]
    assert len(rej) >= 4
    assert {case[n].model for n in rej} == {"SIMPLE_PINHOLE", "SIMPLE_RADIAL"}
    assert {case[n].flags for n in rej} >= {0, 1, 3}
    assert any(case[n].tz < 0 for n in rej)
    for n in NAMES:                                              # (behind the camera means behind the camera)
        if case[n].tz < 0:
            pb = PC.solved(n)[0]
            R = pb["ext0"][pb["frame"]]
            z = pb["points"] @ R[2, :3] + R[2, 3]
            assert (z[pb["mask"][pb["frame"]]] < 0).sum() >= 100
    # every termination, and cap / gradient / parameter / radius also after iteration 0
    assert {summ[n]["termination"] for n in NAMES} == set(PC.TERMINATION)
    for code in (0, 1, 3, 4):
        assert any(summ[n]["termination"] == code and summ[n]["num_iterations"] > 0 and case[n].finite for n in NAMES), code
    assert any(summ[n]["termination"] == 4 and summ[n]["num_unsuccessful_steps"] > 0 for n in NAMES)
    assert any(summ[n]["termination"] == 1 and summ[n]["num_successful_steps"] > 0 for n in NAMES)
    # invalid steps (no candidate at all) and a NaN cost
    assert any(summ[n]["termination"] == 5 and summ[n]["num_unsuccessful_steps"] >= 3 for n in NAMES)
    assert np.isnan(summ["nan_point"]["final_cost"]) and summ["nan_point"]["termination"] == 1
    # inlier counts out of 800 for pose-only or full refinement, and P itself
    counts = {}
    for n in NAMES:
        pb = PC.solved(n)[0]
        counts.setdefault(pb["mask"].shape[1], set()).add(int(pb["mask"][pb["frame"]].sum()))
    assert counts[800] >= {0, 1, 2, 3, 5, 63, 64, 65, 255, 256, 257}
    assert all(counts.get(P) == {P} for P in (0, 1, 3, 70))
    # fewer observations than unknowns
    assert any(2 * int(PC.solved(n)[0]["mask"][PC.solved(n)[0]["frame"]].sum()) < summ[n]["n_reduced"]
               and summ[n]["num_successful_steps"] > 0 for n in NAMES)
    # losses
    assert {case[n].loss for n in NAMES} == {0, 1, 2, 3}
    assert any(case[n].loss == 1 and case[n].scale != 1.0 for n in NAMES)
    # track precisions, SIMPLE_PINHOLE with bit 1 set (n_reduced stays 7 / 6), non-finite data
    assert {case[n].tracks for n in NAMES} == {"f32", "f64"}
    assert summ["easy_pinhole_bit1"]["n_reduced"] == 7 and summ["easy_pinhole_bit1_only"]["n_reduced"] == 6
    assert any(case[n].inf_obs for n in NAMES) and any(case[n].nan_pt for n in NAMES)
    # every field of vgg_ba_options the kernel reads is set by some case (overlap_factorization is the bundle adjuster's)
    fields = {k for n in NAMES for k, _ in case[n].opt}
    assert fields == {f for f, _ in OB.Options._fields_}, {f for f, _ in OB.Options._fields_} - fields


@pytest.mark.parametrize("name", [c.name for c in PC.CASES if c.opt])
def test_option_case_differs_from_its_twin(name):
    """An option that changes nothing tests nothing: the oracle's summary or final state under the option differs from the
    same problem under the twin's options."""
    c = PC.BY_NAME[name]
    assert c.twin in PC.BY_NAME
    t = PC.BY_NAME[c.twin]
    assert (t.model, t.flags, t.frame, t.pert, t.n, t.P, t.loss, t.scale, t.tracks, t.tz, t.inf_obs, t.nan_pt) == \
           (c.model, c.flags, c.frame, c.pert, c.n, c.P, c.loss, c.scale, c.tracks, c.tz, c.inf_obs, c.nan_pt)
    # (the twin differs in the options under test only: the jacobi_scaling cases keep their clamp)
    assert set(dict(t.opt)) <= set(dict(c.opt)) and all(dict(c.opt)[k] == v for k, v in t.opt)
    assert PC.differs_from_twin(name)


def test_jacobi_scaling_alone_changes_nothing():
    """Why `jacobi_scaling = 0` is only tested next to a clamp: with the damping taken from diag(J^T J) the scaling cancels."""
    c = PC.BY_NAME["hard_radial_fk"]
    pb, ext, intr, summ = PC.solved(c.name)
    o = PC.default_options()
    o.jacobi_scaling = 0
    e, p, s = PC.solve(c, pb, options=o)
    assert all(s[k] == summ[k] for k in PC.INT_KEYS)
    np.testing.assert_allclose(e, ext, atol=1e-9)
    np.testing.assert_allclose(p, intr, rtol=1e-9, atol=1e-10)


def test_float64_cases_need_all_64_bits():
    """The float64 table cases are not float32 numbers in disguise: with the tracks rounded to float32 the oracle's final
    cost moves by more than a hundred times the bar the GPU suite holds it to."""
    for name in ("f64_tracks", "f64_tracks_hard_pinhole"):
        pb, _, _, summ = PC.solved(name)
        assert pb["tracks"].dtype == np.float64
        _, _, s32 = PC.solve(PC.BY_NAME[name], dict(pb, tracks=pb["tracks"].astype(np.float32)))
        assert abs(s32["final_cost"] - summ["final_cost"]) > 1e-7 * summ["final_cost"]


def _above_the_floor(got):
    """An exact fit (final cost below 1e-9 of the initial cost) ends on a cost that is the rounding of the pixel coordinates:
    1e-10 px^2 from residuals known to 1e-13 px, so the two derivations cannot agree on it to the 1e-10 relative `_compare`
    asks of every logged cost.  -> (`got` cut before the first iteration either side logs below that floor, with the last
    cost above it as the final cost; the floor).  `_compare` then holds every iteration above the floor to its usual bars."""
    floor = 1e-9 * got["first"]["initial_cost"]
    pairs = list(zip(got["first"]["iterations"], got["second"]["iterations"]))
    keep = next(i for i, (u, v) in enumerate(pairs) if min(u["cost"], v["cost"]) < floor)
    cut = dict(got)
    for side in ("first", "second"):
        its = got[side]["iterations"][:keep]
        cut[side] = dict(got[side], iterations=its, final_cost=its[-1]["cost"])
    return cut, floor


@pytest.mark.parametrize("name", [c.name for c in PC.CASES if c.finite and not (c.n == 0 or c.P == 0)])
def test_second_derivation_walks_the_same_trajectory(monkeypatch, name):
    """oracle/ba_oracle.c and oracle/ba_autograd.py on the case, held to `_compare` of tests/test_oracle_ba_second.py as it
    stands.  Exact fits: `_compare` on the iterations above the rounding floor (`_above_the_floor`), then both final costs
    below the floor, the same integer summary, and the final state inside `_compare`'s own bar (it checks the state of
    the uncut solve)."""
    c = PC.BY_NAME[name]
    pb = PC.build(c)
    got = _both(monkeypatch, lambda: PC.solve(c, pb))
    if not PC.is_exact_fit(got["first"]):
        _compare(got, min_compared=3)
        return
    cut, floor = _above_the_floor(got)
    assert len(cut["first"]["iterations"]) >= 2                  # (iteration 0 and at least one step are compared)
    _compare(cut, min_compared=min(3, len(cut["first"]["iterations"])))
    assert got["first"]["final_cost"] < floor and got["second"]["final_cost"] < floor
    assert all(got["first"][k] == got["second"][k] for k in PC.INT_KEYS)
