"""The exact model of tests/linearize_model.py against what the compiled reference's own vertex and edge classes computed
on the fixtures of tests/golden/linearize/ (CPU only).

Expectation, error, chi^2 and the states after Operator_Plus / Operator_Minus are the same functions evaluated twice: the
project's 1e-10, rel-inf.  So are the SE(2) Jacobians, which the reference has in closed form.  Its SE(3) and camera-point
Jacobians are forward differences with a step of 1e-9 (3DSolverBase.h:1331-1371, BASolverBase.h:577-619): there the gap to
the exact derivative is the reference's own differencing error.  It is printed (and recorded in DESIGN.md section 4.9), and
the only assertion is a guard against a convention error -- a wrong sign, a transposed block, a perturbation on the wrong
side are errors of order 1, the guard is 1e-5 -- over every edge."""
import numpy as np
import pytest

import linearize_model as M
from golden_util import rel_inf

TOL = 1e-10
CONVENTION_GUARD = 1e-5


@pytest.mark.parametrize("kind", M.KINDS)
def test_expectation_error_and_chi2(kind):
    fx = M.load_fixture(kind)
    h, err, _, _ = M.fixture_model(kind)
    assert rel_inf(h, fx["expectation"]) < TOL
    assert rel_inf(err, fx["err"]) < TOL
    assert np.abs(fx["err"]).max() > 1e-3          # the states were not initialized from the edges
    chi2 = M.chi2(err, fx["sigma_inv"])
    assert abs(chi2 - float(fx["chi2"])) < TOL * abs(float(fx["chi2"]))


@pytest.mark.parametrize("kind", M.KINDS)
def test_plus_and_minus(kind):
    fx = M.load_fixture(kind)
    kinds = M.vertex_kinds(kind, fx)
    assert rel_inf(M.state_plus(kinds, fx["state"], fx["cumsum"], fx["dx"]), fx["state_plus"]) < TOL
    assert rel_inf(M.state_plus(kinds, fx["state"], fx["cumsum"], fx["dx"], -1.0), fx["state_minus"]) < TOL
    assert rel_inf(fx["state_plus"], fx["state"]) > 1e-4


def test_se2_jacobians():
    fx = M.load_fixture("se2")
    _, _, J0, J1 = M.fixture_model("se2")
    assert rel_inf(J0, fx["J0"]) < TOL and rel_inf(J1, fx["J1"]) < TOL


@pytest.mark.parametrize("kind", ["se3", "ba"])
def test_forward_difference_gap(kind):
    """max |J_fixture - J_model| / max |J_model| per type: the reference's forward-difference error.  Measured here:
    SE(3) 7.5e-7 (J0), 2.2e-6 (J1); camera-point 6.5e-7 (J0), 1.5e-6 (J1)."""
    fx = M.load_fixture(kind)
    _, _, J0, J1 = M.fixture_model(kind)
    assert J0.shape == fx["J0"].shape and J1.shape == fx["J1"].shape and not np.isnan(J0).any() and not np.isnan(J1).any()
    for name, J, ref in (("J0", J0, fx["J0"]), ("J1", J1, fx["J1"])):
        gap = float(np.abs(ref - J).max() / np.abs(J).max())
        print(f"linearize_{kind} {name}: reference forward-difference gap {gap:.3e} (max |J_model| {np.abs(J).max():.3e})")
        assert gap < CONVENTION_GUARD, (kind, name, gap)


def test_se3_fixture_covers_the_rotation_cases():
    fx = M.load_fixture("se3")
    norms = np.linalg.norm(fx["state"].reshape(-1, 6)[:, 3:], axis=1)
    assert norms[0] == 0 and np.isclose(norms[1], 1e-9, rtol=1e-9, atol=0) and np.isclose(norms[2], 1e-5) and np.isclose(norms[3], 1e-3)
    assert ((norms > 1) & (norms < 3)).sum() >= 5 and sorted(norms[norms > np.pi].round(12)) == [3.5, 5.0]
    limit = np.pi - 0.2
    assert np.linalg.norm(fx["expectation"][:, 3:], axis=1).max() < limit and np.linalg.norm(fx["err"][:, 3:], axis=1).max() < limit
    assert (fx["v0"] > fx["v1"]).sum() == 4 and len(fx["v0"]) == 55


def test_se2_fixture_wraps():
    fx = M.load_fixture("se2")
    assert (np.abs(fx["z"][:, 2] - fx["expectation"][:, 2]) > np.pi).sum() >= 3
    assert np.abs(fx["err"][:, 2]).max() < 1.0
