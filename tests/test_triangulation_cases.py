"""CPU: the long-double triangulation reference of tests/triangulation_cases.py checked by itself, against the reference
project's recorded output (tests/golden/tri_regimes_*.npz, oracle/gen_golden_tri_regimes.py) and against the mild goldens the
suite already had.  Every test prints its figures before it asserts."""
import numpy as np
import pytest

from tests import triangulation_cases as C


def _golden(golden_dir, name):
    with np.load(f"{golden_dir}/{name}.npz", allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def test_jacobi_against_lapack():
    rng = np.random.default_rng(0)
    B = rng.standard_normal((500, 6, 4))
    A = np.einsum("bki,bkj->bij", B, B)
    A[250:] = np.einsum("bki,bkj->bij", B[250:, :3], B[250:, :3])              # rank 3: a zero eigenvalue
    w, V = C.jacobi_eigh4(A.astype(C.LD))
    wl, _ = np.linalg.eigh(A)
    res = np.abs(np.einsum("bij,bjk->bik", A, V.astype(np.float64)) - V.astype(np.float64) * w.astype(np.float64)[:, None, :]).max()
    orth = np.abs(np.einsum("bji,bjk->bik", V, V) - np.eye(4)).max()
    print(f"\neigenvalues vs LAPACK {np.abs(w.astype(np.float64) - wl).max():.2e}, residual {res:.2e}, orthogonality {float(orth):.2e}")
    assert np.abs(w.astype(np.float64) - wl).max() <= 1e-13 * wl.max() and res <= 1e-13 * wl.max() and orth <= 1e-17


@pytest.mark.parametrize("name", C.NAMES)
def test_long_double_agrees_with_the_reference_project(name):
    """Pins the semantics of the restatement: on every admitted track the reference project's own float64 run has the same
    mask and count, and its point within the point bound -- the rule of the device's bound, built from what float64 does
    with the reference's own eigen-solver (LAPACK; see triangulation_cases.py on dev64_lapack)."""
    g = C.load(name)
    adm = g["ld_admitted"]
    bound = max(C.POINT_FLOOR, C.MARGIN * float(g["ld_dev64_lapack"]))
    cmp = adm & (g["ld_num"] >= 2)
    dev = C.rel_point_distance(g["ref_points"], g["ld_points"], float(g["size"]))
    worst = float(dev[cmp].max()) if cmp.any() else 0.0
    left_out = 1 - adm.mean()
    print(f"\n{name}: N {len(adm)} left out {left_out:.4f} (cap {C.CAP}) | delta {float(g['ld_delta']):.2e} decision dev64 "
          f"{float(g['ld_decision_dev64']):.2e} | mask bits differing on admitted {int((g['ref_mask'][adm] != g['ld_mask'][adm]).sum())}, "
          f"on the rest {int((g['ref_mask'][~adm] != g['ld_mask'][~adm]).sum())} | reference point deviation {worst:.3e} "
          f"(bound {bound:.3e}, dev64 {float(g['ld_dev64']):.3e}, with LAPACK {float(g['ld_dev64_lapack']):.3e}) | thresholds {g['ld_thresholds']}")
    assert left_out <= C.CAP
    assert float(g["ld_delta"]) == max(C.DELTA_FLOOR, C.MARGIN * float(g["ld_decision_dev64"]))
    assert np.array_equal(g["ref_mask"][adm], g["ld_mask"][adm]) and np.array_equal(g["ref_num"][adm], g["ld_num"][adm])
    assert worst <= bound
    # the chunk thresholds: below 2 pi exactly where the case says that every hypothesis has an inlier; what float64 makes of
    # the multi-chunk ones is within the bound the device is held to
    if name in C.RETHRESHOLD:
        assert (g["ld_thresholds"] < 2 * np.pi).all()
    elif name != "exact":
        assert (g["ld_thresholds"] == 2 * np.pi + 1e-6).all()
    if name in C.MULTI_CHUNK:
        assert len(g["ld_thresholds"]) == 3
        assert (np.abs(g["ld_thresholds64"] - g["ld_thresholds"]) <= C.THRESHOLD_RTOL * g["ld_thresholds"]).all()


@pytest.mark.parametrize("name", C.NAMES)
def test_fixture_is_what_the_recipe_produces(name):
    """The case table still builds the recorded inputs, and the long-double half of the recipe, run again on a slice of the
    tracks, gives the recorded bits."""
    g = C.load(name)
    built = C.build(name)
    case = C.case_from_fixture(name, g)
    for k in ("ext", "tn", "vis"):
        assert np.allclose(built[k], case[k], rtol=0, atol=1e-12 * float(g["size"]))
    assert (built["score"] is None) == (case["score"] is None) and built["seed"] == case["seed"]
    N = case["tn"].shape[1]
    tracks = np.arange(0, N, 32 if N > 1000 else 4)
    r = C.reference(case, C.draw_pairs(case), tracks, delta=g["ld_delta"], bound=max(C.POINT_FLOOR, C.MARGIN * float(g["ld_dev64"])),
                    thresholds=g["ld_thresholds"])
    same = {k: np.array_equal(r[k], g[f"ld_{k}"][tracks], equal_nan=True) for k in ("points", "num", "mask", "admitted")}
    print(f"\n{name}: {len(tracks)} of {N} tracks recomputed: identical {same}")
    assert all(same.values())


@pytest.mark.parametrize("name", ["tri_tracks_s8_all_pairs", "tri_tracks_s30_it128"])
def test_long_double_agrees_with_the_mild_goldens(golden_dir, name):
    g = _golden(golden_dir, name)
    S = g["extrinsics"].shape[0]
    case = dict(ext=g["extrinsics"], tn=g["tracks_normalized"].astype(np.float64), vis=g["vis"], score=g["score"],
                iters=int(g["max_ransac_iters"]), max_pts=int(g["max_tri_points_num"]), size=1.0)
    comb = C.all_pairs(S)
    pairs = [comb if case["iters"] > len(comb) else comb[g[f"randperm_{i}"][:case["iters"]]] for i in range(max(1, int(g["n_draws"])))]
    r = C.reference(case, pairs)
    adm = r["admitted"]
    cmp = adm & (r["num"] >= 2)
    worst = float(C.rel_point_distance(g["points"], r["points"], 1.0)[cmp].max())
    bound = max(C.POINT_FLOOR, C.MARGIN * r["dev64_lapack"])
    print(f"\n{name}: left out {1 - adm.mean():.4f} | mask bits differing on admitted {int((g['inlier_mask'][adm] != r['mask'][adm]).sum())} "
          f"| golden point deviation {worst:.3e} (bound {bound:.3e})")
    assert 1 - adm.mean() <= C.CAP
    assert np.array_equal(g["inlier_mask"][adm], r["mask"][adm]) and np.array_equal(g["inlier_num"][adm], r["num"][adm])
    assert worst <= bound


def _pair_source(group, g):
    return g if group == "pair_sweep" else C.load(group)


def test_pair_sweep_lapack_constant():
    """PAIR_C_LAPACK is what float64 LAPACK reaches on the sweep (it moves a little with the LAPACK build; the bound for the
    device is ten times the recorded value and LAPACK itself has to stay inside it)."""
    g = C.load("pair_sweep")
    f64 = C.pair_reference(g["ext"], g["tn"], np.float64)
    _, V = np.linalg.eigh(f64["A"])
    with np.errstate(all="ignore"):
        X = V[..., :3, 0] / V[..., 3:, 0]
        gap, unit = C.pair_condition(g["ld_lam"])
        ratio = C.direction_angle(X, g["ld_points"]) / unit
    big = gap >= C.GAP_MIN
    par = np.rad2deg(np.exp(np.linspace(np.log(np.deg2rad(30.0)), np.log(1e-7), len(gap))))
    print(f"\npair_sweep: {big.size} inputs, parallax {par[0]:.1f} .. {par[-1]:.1e} degrees, {int(big.sum())} with a relative gap >= "
          f"{C.GAP_MIN:g} | LAPACK reaches {np.nanmax(ratio[big]):.4f} (recorded {C.PAIR_C_LAPACK}, bound {C.PAIR_C:g})")
    assert big.sum() >= 1800 and (~big).sum() >= 50           # the sweep covers both sides of the gap
    assert np.nanmax(ratio[big]) <= C.PAIR_C and C.PAIR_C == 10 * C.PAIR_C_LAPACK


@pytest.mark.parametrize("group", C.PAIR_GROUPS)
def test_pair_reference_agrees_with_the_reference_project(group):
    g = C.load(C.pair_name(group))
    src = _pair_source(group, g)
    gap, unit = C.pair_condition(g["ld_lam"])
    big = gap >= C.GAP_MIN
    with np.errstate(all="ignore"):
        ratio = C.direction_angle(g["ref_points"], g["ld_points"]) / unit
    ld = C.pair_reference(src["ext"][:3], src["tn"][:3])
    same = np.array_equal(ld["points"].astype(np.float64), g["ld_points"][:2], equal_nan=True)
    print(f"\n{group}: {big.size} inputs, {int(big.sum())} above the gap | reference project reaches {np.nanmax(ratio[big]):.4f} "
          f"(bound {C.PAIR_C:g}) | first two frames recomputed identical: {same}")
    assert np.nanmax(ratio[big]) <= C.PAIR_C and not np.isnan(ratio[big]).any()
    assert same
