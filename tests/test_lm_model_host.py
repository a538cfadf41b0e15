"""The model of the device-decided Levenberg-Marquardt loop (tests/lm_model.py) on the three fixtures of tests/golden/linearize/,
without a GPU: the accept patterns the GPU tests rely on, the condition on the inputs that no compared decision hangs on
rounding, and how far the way of solving the linear system (Cholesky or LU) moves the trajectory -- the figure the GPU tests'
tolerances are 100 times of."""
import numpy as np
import pytest

import linearize_model as M
import lm_model as L


def pattern(result):
    return "".join(str(int(a)) for a in result["trace"][:, L.T_ACCEPTED])


def test_accept_patterns():
    se2, se3, ba = (L.fixture_run(k) for k in ("se2", "se3", "ba"))
    assert pattern(se2) == "1" * 14 and se2["scalars"][L.STATUS] == L.RUNNING
    # SE(3): two accepted, five rejected in a row (nu reaches 64), then accepted
    assert pattern(se3) == "11000001111111" and se3["scalars"][L.N_REJECTED] == 5 and se3["scalars"][L.EXTRA_LEFT] == 5
    assert se3["trace"][6, L.T_NU] == 64.0 and se3["trace"][7, L.T_NU] == 2.0
    # BA with f_min_dx_norm = 1e-6: four steps, converged in the fifth round; the three rounds behind it are inert
    assert pattern(ba) == "11110" and list(ba["trace"][:, L.T_STATUS]) == [0, 0, 0, 0, L.CONVERGED]
    assert ba["scalars"][L.N_ROUNDS] == 5 and len(ba["states"]) == 9 and all(np.array_equal(ba["states"][4], s) for s in ba["states"][5:])
    assert all(np.array_equal(ba["scalars_after"][4], s) for s in ba["scalars_after"][5:])
    dx = ba["trace"][:, L.T_DX_NORM]
    assert np.all(dx[:4] > 1e-6) and dx[4] < 1e-6


@pytest.mark.parametrize("kind", M.KINDS)
def test_no_compared_decision_hangs_on_rounding(kind):
    """A condition on the inputs: every round that forms a gain ratio has |rho| >= 1e-3, far from the rho > 0 test."""
    r = L.fixture_run(kind)
    rho = r["trace"][:L.compared_rounds(r), L.T_RHO]
    print(f"lm_model {kind}: |rho| over the compared rounds {np.abs(rho).min():.3g} .. {np.abs(rho).max():.3g}")
    assert len(rho) >= 4 and np.all(np.abs(rho) >= 1e-3)


@pytest.mark.parametrize("kind", M.KINDS)
def test_sensitivity_to_the_linear_solve(kind):
    """Cholesky against LU: the same decisions, and figures that differ by rounding carried through the loop (printed; the
    GPU tests allow 100 times as much, and not below 1e-10)."""
    a, b = L.fixture_run(kind, "chol"), L.fixture_run(kind, "lu")
    assert pattern(a) == pattern(b) and np.array_equal(a["trace"][:, L.T_STATUS], b["trace"][:, L.T_STATUS])
    s = L.sensitivity(kind)
    print(f"lm_model {kind}: Cholesky against LU, relative: " + ", ".join(f"{q} {s[q]:.2e}" for q in L.QUANTITIES))
    assert s["chi2"] < 1e-12 and s["state"] < 1e-12 and s["alpha"] < 1e-8


@pytest.mark.parametrize("kind", M.KINDS)
def test_against_the_reference(kind):
    """The reference's CNonlinearSolver_Lambda_LM on the same graphs from the same states with its own anchor
    (tests/golden/lm/): the model takes as many iterations for every n_max (BA: up to its convergence in the fifth round; past
    it rho is 0 / 0 on both sides and nothing is compared), and ends where the reference does but for the reference's
    forward-difference Jacobians.  The gap is printed; beyond 1e-5 of chi^2 something other than differencing would differ."""
    ref, runs = L.load_reference(kind), L.reference_runs(kind)
    for n_max, r in enumerate(runs, 1):
        if kind == "ba" and n_max > 5:
            assert r["scalars"][L.STATUS] == L.CONVERGED and r["scalars"][L.N_ROUNDS] == 5
            continue
        chi2, state = ref["chi2"][n_max - 1], ref["states"][n_max - 1]
        gap_chi2 = abs(r["scalars"][L.LAST_ERROR] - chi2) / chi2
        gap_state = np.abs(r["state"] - state).max() / np.abs(state).max()
        print(f"lm_model {kind} Optimize({n_max}): {int(r['scalars'][L.N_ROUNDS])} iterations, chi2 from the reference by {gap_chi2:.2e}, "
              f"the state by {gap_state:.2e}")
        assert r["scalars"][L.N_ROUNDS] == ref["n_iterations"][n_max - 1]
        assert gap_chi2 < 1e-5 and gap_state < 1e-5
        if kind == "se2":                                # closed-form Jacobians on both sides
            assert gap_chi2 < 1e-10 and gap_state < 1e-10
    if kind == "se3":                                    # the budget: Optimize(3) takes nine solves, six of them rejected
        s = runs[2]["scalars"]
        assert (s[L.STATUS], s[L.N_ROUNDS], s[L.N_ACCEPTED], s[L.N_REJECTED], s[L.EXTRA_LEFT]) == (L.BUDGET, 9, 3, 6, 4)


def test_budget_of_extra_iterations():
    """Optimize(3) on the SE(3) fixture: the five rejected steps are granted an iteration each, the eighth solve is the third
    accepted step and uses the budget up."""
    r = L.run("se3", 13, n_max_iterations=3, n_extra_on_reject=10)
    s = r["scalars"]
    assert (s[L.STATUS], s[L.N_ROUNDS], s[L.N_ACCEPTED], s[L.N_REJECTED], s[L.EXTRA_LEFT], s[L.ROUNDS_LEFT]) == (L.BUDGET, 8, 3, 5, 5, 0)
    assert len(r["trace"]) == 8 and np.array_equal(r["states"][8], r["states"][13])


def test_decide_rule():
    """The rule on crafted scalars: the cap 1 - t^3 against 1/3, a NaN rejects, the order of the breaks."""
    def block(**kw):
        s = L.begin(2.0, 10.0, 1e-6, 5, 2)
        s[L.DX_DX], s[L.DX_ETA] = 1.0, 2.0            # the denominator: alpha * 1 + 2 = 4
        for k, v in kw.items():
            s[getattr(L, k)] = v
        return s
    s = block()
    L.decide(s, False, [10.0 - 4 * 0.9])              # rho = 0.9: 1 - 0.8^3 = 0.488 > 1/3
    assert s[L.ACCEPTED] == 1 and abs(s[L.RHO] - 0.9) < 1e-15 and abs(s[L.ALPHA] - 2 * (1 - 0.8 ** 3)) < 1e-15 and s[L.ROUNDS_LEFT] == 4
    s = block()
    L.decide(s, False, [10.0 - 4 * 1e-3])             # rho = 1e-3: the cap is 1 - (-0.998)^3 = 1.994, not 1/3
    assert s[L.ACCEPTED] == 1 and abs(s[L.ALPHA] - 2 * (1 + 0.998 ** 3)) < 1e-12
    s = block()
    L.decide(s, False, [10.0 - 4 * 1.5])              # rho = 1.5: 1 - 8 < 1/3
    assert s[L.ALPHA] == 2 / 3.0
    for chi2 in (10.0, 11.0, float("nan")):           # rho = 0, rho < 0, NaN
        s = block()
        L.decide(s, False, [chi2])
        assert (s[L.ACCEPTED], s[L.ALPHA], s[L.NU], s[L.LAST_ERROR], s[L.EXTRA_LEFT], s[L.ROUNDS_LEFT]) == (0, 4.0, 4.0, 10.0, 1, 5)
    s = block(DX_DX=1e-14)
    L.decide(s, False, [1.0])
    assert (s[L.STATUS], s[L.ACCEPTED], s[L.ALPHA], s[L.ROUNDS_LEFT]) == (L.CONVERGED, 0, 2.0, 5)
    s = block(DX_DX=1e-14)
    L.decide(s, True, [1.0])                          # the flag comes first
    assert s[L.STATUS] == L.NOT_POSDEF
    s = block(ROUNDS_LEFT=1, EXTRA_LEFT=0)
    L.decide(s, False, [11.0])
    assert (s[L.STATUS], s[L.ROUNDS_LEFT], s[L.N_REJECTED]) == (L.BUDGET, 0, 1)
    before = s.copy()
    L.decide(s, False, [1.0])                         # status set: nothing moves
    assert np.array_equal(s, before)
