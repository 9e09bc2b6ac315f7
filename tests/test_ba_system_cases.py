"""The long-double reference of the bundle adjustment's intermediates (tests/ba_system_cases.py) against the C oracle, on the
CPU: two derivations that share nothing -- autograd Jacobians + dense long-double algebra against analytic Jacobians + the
oracle's own Schur elimination in double -- before any kernel is compared with the first (tests/test_gpu_ba_system.py)."""
import numpy as np
import pytest

from tests import ba_system_cases as SC


@pytest.mark.parametrize("name", list(SC.CASES))
def test_reference_matches_the_c_oracle(name):
    """Reduced system S | rhs = bao_debug_dump_system's of a one-iteration oracle.ba.solve_csr on the same arrays; the
    reference's first step reproduces that solve's iterations[1].  The case reaches its edge (on the CPU the work list is
    sized for another device, its tiles and entries are the same)."""
    prob = SC.compile_case(name)
    SC.check_edges(name, prob)
    a = SC.host_arrays(prob, SC.CASES[name])
    R = SC.reference(name, a)
    lhs, rhs, summ = SC.oracle_first_iteration(a)
    ref, pb = R.ref, R.pb
    n = pb.n_red
    assert summ["n_reduced"] == n and lhs.shape == (n, n) and len(summ["iterations"]) == 2
    act = pb.active[:n]
    diag = np.where(act, np.diag(ref.S), 0).astype(np.float64)
    e_S = max(SC.normalised_error(lhs, ref.S, diag), SC.normalised_error(lhs.T, ref.S, diag))      # (the dump is full symmetric)
    e_rhs = SC.relative_to_max(rhs[act], ref.rhs[act])
    it = summ["iterations"][1]
    rel = lambda x, y: abs(float(x) - y) / abs(y)
    e_step = {k: rel(getattr(ref, k), it[k]) for k in ("cost_change", "step_norm", "relative_decrease")}
    print(f"{name}: n = {n}, {len(pb.obs_cam)} observations, reference in {R.seconds:.1f} s; against the oracle: S {e_S:.2e}, "
          f"rhs {e_rhs:.2e}, " + ", ".join(f"{k} {v:.2e}" for k, v in e_step.items()))
    print(f"{name}: float64 evaluation against long double: " + ", ".join(f"{k} {v:.1e}" for k, v in R.dev.items()))
    # the oracle's inactive columns: unit diagonal, zero right-hand side; the reference's: the damping of a zero column
    ina = np.nonzero(~act)[0]
    assert (lhs[ina, ina] == 1.0).all() and (rhs[ina] == 0.0).all()
    so = R.so
    assert (np.diag(ref.S)[ina] == np.longdouble(so.min_lm_diagonal) / np.longdouble(so.initial_trust_region_radius)).all()
    off = ref.S.copy()
    off[np.arange(n), np.arange(n)] = 0
    assert (off[ina] == 0).all() and (off[:, ina] == 0).all() and (ref.rhs[ina] == 0).all()
    assert it["successful"] and float(ref.relative_decrease) > so.min_relative_decrease
    assert abs(float(ref.cost_x) - summ["initial_cost"]) <= 1e-13 * summ["initial_cost"]
    assert e_S <= SC.ORACLE_SYSTEM_BOUND and e_rhs <= SC.ORACLE_RHS_BOUND, (e_S, e_rhs)
    assert max(e_step.values()) <= SC.ORACLE_STEP_BOUND, e_step
