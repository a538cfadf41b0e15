"""The exact model of tests/landmark_model.py against what the compiled reference's own vertex and edge classes computed on
the fixtures of tests/golden/landmark/ (CPU only).

Expectation, error, chi^2 and the states after Operator_Plus / Operator_Minus are the same functions evaluated twice: the
project's 1e-10, rel-inf.  So are the 2D Jacobians, which the reference has in closed form -- the three close edges with
the range clamp included -- and the model's closed form is autograd's derivative on the regular edges.  The reference's 3D
and stereo Jacobians are forward differences with a step of 1e-9 (3DSolverBase.h:1602-1637, BASolverBase.h:801-840): the
model's exact derivatives lie within that differencing error of them, max |J_model - J_ref| <= 1e-5 max |J_model|; the gap
is printed."""
import numpy as np
import pytest
import torch

import landmark_model as L
from golden_util import rel_inf

TOL = 1e-10
FORWARD_DIFFERENCE = 1e-5


@pytest.mark.parametrize("name", L.NAMES)
def test_expectation_error_and_chi2(name):
    fx = L.load_fixture(name)
    h, err, _, _ = L.fixture_model(name)
    assert rel_inf(h, fx["expectation"]) < TOL
    assert rel_inf(err, fx["err"]) < TOL
    assert np.abs(fx["err"]).max() > 1e-3          # the states were not initialized from the edges
    chi2 = L.M.chi2(err, fx["sigma_inv"])
    assert abs(chi2 - float(fx["chi2"])) < TOL * abs(float(fx["chi2"]))


@pytest.mark.parametrize("name", L.NAMES)
def test_plus_and_minus(name):
    fx = L.load_fixture(name)
    kinds = L.vertex_kinds(name, fx)
    assert rel_inf(L.M.state_plus(kinds, fx["state"], fx["cumsum"], fx["dx"]), fx["state_plus"]) < TOL
    assert rel_inf(L.M.state_plus(kinds, fx["state"], fx["cumsum"], fx["dx"], -1.0), fx["state_minus"]) < TOL
    assert rel_inf(fx["state_plus"], fx["state"]) > 1e-4


def test_lm2d_closed_form_is_the_derivative_on_the_regular_edges():
    fx = L.load_fixture("lm2d")
    n = int(fx["n_regular"])
    state = torch.from_numpy(fx["state"])
    x0 = torch.stack([state[o:o + 3] for o in fx["cumsum"][fx["v0"][:n]]])
    x1 = torch.stack([state[o:o + 2] for o in fx["cumsum"][fx["v1"][:n]]])
    J0, J1 = L.lm2d_jacobians(x0.numpy(), x1.numpy())
    J0_a, J1_a = L.lm2d_jacobians_autograd(x0, x1)
    assert rel_inf(J0, J0_a.numpy()) < TOL and rel_inf(J1, J1_a.numpy()) < TOL


def test_lm2d_jacobians_close_edges_included():
    fx = L.load_fixture("lm2d")
    _, _, J0, J1 = L.fixture_model("lm2d")
    assert len(J0) == len(fx["v0"]) == int(fx["n_regular"]) + 3
    assert rel_inf(J0, fx["J0"]) < TOL and rel_inf(J1, fx["J1"]) < TOL
    assert rel_inf(J0[-3:], fx["J0"][-3:]) < TOL and rel_inf(J1[-3:], fx["J1"][-3:]) < TOL   # (their own largest entry: 1e5 at 5e-6)
    assert not np.isnan(fx["J0"]).any() and not np.isnan(fx["J1"]).any()


@pytest.mark.parametrize("name", ["lm3d", "stereo"])
def test_forward_difference_gap(name):
    """max |J_model - J_fixture| / max |J_model|: the reference's forward-difference error.  Measured here: lm3d 6.9e-7 (J0),
    1.1e-6 (J1); stereo 7.8e-7 (J0), 1.6e-6 (J1)."""
    fx = L.load_fixture(name)
    _, _, J0, J1 = L.fixture_model(name)
    assert J0.shape == fx["J0"].shape and J1.shape == fx["J1"].shape and not np.isnan(J0).any() and not np.isnan(J1).any()
    for which, J, ref in (("J0", J0, fx["J0"]), ("J1", J1, fx["J1"])):
        gap = float(np.abs(J - ref).max() / np.abs(J).max())
        print(f"landmark_{name} {which}: reference forward-difference gap {gap:.3e} (max |J_model| {np.abs(J).max():.3e})")
        assert np.abs(J - ref).max() <= FORWARD_DIFFERENCE * np.abs(J).max(), (name, which, gap)


def test_lm2d_fixture_is_what_the_tests_need():
    fx = L.load_fixture("lm2d")
    n_poses, n_regular = int(fx["n_poses"]), int(fx["n_regular"])
    assert n_poses == 30 and len(fx["cumsum"]) - 1 == 42 and list(np.diff(fx["cumsum"])) == [3] * 30 + [2] * 12
    assert len(fx["a_v0"]) > 29 and (np.abs(fx["z"][:, 1] - fx["expectation"][:, 1]) > np.pi).sum() >= 3
    seen = np.bincount(fx["v1"] - n_poses, minlength=12)
    assert seen.min() >= 3 and seen.max() <= 6
    state = fx["state"]
    d = [np.linalg.norm(state[fx["cumsum"][b]:fx["cumsum"][b] + 2] - state[fx["cumsum"][a]:fx["cumsum"][a] + 2])
         for a, b in zip(fx["v0"][-3:], fx["v1"][-3:])]
    assert d[0] == 0 and abs(d[1] - 5e-6) < 1e-14 and abs(d[2] - 2e-5) < 1e-14     # (coordinates near 30: spaced 3.6e-15)
    assert all((fx["v1"][:n_regular] == b).sum() >= 2 for b in fx["v1"][-3:])
    assert list(fx["expectation"][-3:, 0] == 1e-5) == [True, True, False]


def test_lm3d_fixture_is_what_the_tests_need():
    fx = L.load_fixture("lm3d")
    assert int(fx["n_first_pose"]) == 15 and int(fx["n_poses"]) == 25 and list(np.diff(fx["cumsum"])) == [3] * 15 + [6] * 25
    assert (fx["v0"] > fx["v1"]).all()
    norms = np.linalg.norm(fx["state"][45:].reshape(-1, 6)[:, 3:], axis=1)
    assert norms[0] == 0 and np.isclose(norms[1], 1e-9, rtol=1e-9, atol=0) and np.isclose(norms[2], 1e-5) and np.isclose(norms[3], 1e-3)
    assert (norms > np.pi).sum() >= 1
    assert {15, 16, 17, 18} <= set(fx["v0"].tolist()) and 15 + int(np.argmax(norms > np.pi)) in set(fx["v0"].tolist())


def test_stereo_fixture_is_what_the_tests_need():
    fx = L.load_fixture("stereo")
    K = fx["params"].reshape(-1, 6)
    assert K.shape[0] == 6 and (K[:, 5] == 0).sum() == 1 and K[:, 5].max() == 0.5 and K[K[:, 5] > 0, 5].min() == 0.1
    seen = np.bincount(fx["v1"] - 6, minlength=40)
    assert len(seen) == 40 and seen.min() >= 2 and seen.max() <= 4
    assert len(np.unique(K[:, 0])) == 6 and (K[:, 4] != 0).all()
