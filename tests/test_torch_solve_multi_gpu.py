"""K right-hand sides on one set of values as a differentiable PyTorch operation (torch_solve.solve_multi), in both modes: the
forward rows against ``solve`` row by row, both gradients of loss = sum(W * X) against fp64 dense autograd on the CPU
(dense_from_packed + torch.linalg.solve) to the tolerance tests/test_torch_solve_gpu.py uses for ``solve`` (1e-10 rel-inf), K = 1
against ``solve`` itself, who owns the kept factor and what a backward pass that has lost it costs, a Schur solver with and
without schur_keep, a matrix that is not positive definite, and the argument checks."""
import functools

import numpy as np
import pytest
import torch

from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP, CLinearSolver_Schur_HIP
from slam_plus_plus_amd.torch_solve import solve, solve_multi, dense_from_packed, MAX_COLUMNS
from golden_util import load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-10
K = 5


def rel_inf(got, ref):
    got, ref = got.detach().cpu().numpy(), ref.detach().cpu().numpy()
    return float(np.abs(got - ref).max() / np.abs(ref).max())


@functools.lru_cache(maxsize=None)
def _problem(name, k):
    """(the system, eta[k, n]: row 0 the fixture's eta and seeded normals after it, the weights W[k, n] of the loss)"""
    lam = load_golden(name)[0]
    rng = np.random.default_rng(51)
    eta = rng.standard_normal((k, lam.n_scalars))
    eta[0] = lam.rhs
    return lam, torch.from_numpy(eta), torch.from_numpy(rng.standard_normal((k, lam.n_scalars)))


@functools.lru_cache(maxsize=None)
def _dense_reference(name, k):
    """(X, values gradient, eta gradient) of loss = sum(W * (M(values)^-1 eta^T)^T) by dense autograd on the CPU; computed once."""
    lam, eta, W = _problem(name, k)
    values = torch.from_numpy(lam.values).clone().requires_grad_(True)
    eta = eta.clone().requires_grad_(True)
    X = torch.linalg.solve(dense_from_packed(lam, values), eta.T).T
    (W * X).sum().backward()
    return X.detach(), values.grad, eta.grad


def _device_gradients(solver, name, k, pad=0):
    lam, eta, W = _problem(name, k)
    values = torch.tensor(lam.values, device="cuda", requires_grad=True)
    buf = torch.zeros((k, lam.n_scalars + pad), dtype=torch.float64, device="cuda")
    buf[:, :lam.n_scalars] = eta.cuda()
    eta_dev = buf[:, :lam.n_scalars].detach().requires_grad_(True)
    assert eta_dev.stride(0) == lam.n_scalars + pad
    X = solve_multi(solver, lam, values, eta_dev)
    (W.cuda() * X).sum().backward()
    return X.detach(), values.grad, eta_dev.grad


def _assert_matches_dense(name, k, got, what=""):
    errs = [rel_inf(g, r) for g, r in zip(got, _dense_reference(name, k))]
    print(f"solve_multi {name}, K = {k}{what}: rel-inf of X {errs[0]:.2e}, of the values gradient {errs[1]:.2e}, "
          f"of the eta gradient {errs[2]:.2e}")
    assert max(errs) < TOL


@pytest.mark.parametrize("pad", [0, 3], ids=["packed_rows", "padded_rows"])
@pytest.mark.parametrize("name", ["chain3_n90", "sphere_8x8"])
def test_sparse_mode_forward_and_gradients(name, pad):
    lam, eta, _ = _problem(name, K)
    solver = CLinearSolver_HIP()
    got = _device_gradients(solver, name, K, pad)
    assert got[2].shape == (K, lam.n_scalars) and got[1].shape == lam.values.shape
    _assert_matches_dense(name, K, got, f", row stride n + {pad}")
    assert solver.n_backward_refactorizations == 0                       # all of it on the kept factor
    # the forward rows against solve, row by row
    values = torch.tensor(lam.values, device="cuda")
    rows = torch.stack([solve(solver, lam, values, eta[k].cuda()) for k in range(K)])
    worst = max(rel_inf(got[0][k], rows[k]) for k in range(K))
    print(f"solve_multi {name}: worst rel-inf of a row against solve {worst:.2e}")
    assert worst < TOL and torch.equal(got[0][0], rows[0])               # (row 0 is the factorizing call itself)


def test_one_row_equals_solve():
    name = "chain6_n60"
    lam, eta, W = _problem(name, 1)
    solver = CLinearSolver_HIP()
    X, v_bar, eta_bar = _device_gradients(solver, name, 1)
    values = torch.tensor(lam.values, device="cuda", requires_grad=True)
    eta_dev = eta[0].cuda().requires_grad_(True)
    x = solve(solver, lam, values, eta_dev)
    (W[0].cuda() @ x).backward()
    errs = (rel_inf(v_bar, values.grad), rel_inf(eta_bar[0], eta_dev.grad))
    print(f"solve_multi {name}, K = 1 against solve: values gradient {errs[0]:.2e}, eta gradient {errs[1]:.2e}")
    assert torch.equal(X[0], x.detach()) and max(errs) < TOL


@pytest.mark.parametrize("schur_sparse", [0, 1])
def test_schur_mode_with_the_kept_factor(schur_sparse):
    name = "ba_10x120_band"
    solver = CLinearSolver_Schur_HIP(schur_keep=1, schur_sparse=schur_sparse)
    _assert_matches_dense(name, K, _device_gradients(solver, name, K), f" schur_keep, schur_sparse={schur_sparse}")
    assert solver.n_backward_refactorizations == 0


def test_schur_mode_without_schur_keep_solves_row_by_row():
    name, k = "ba_12x150_venice", 3
    solver = CLinearSolver_Schur_HIP()
    _assert_matches_dense(name, k, _device_gradients(solver, name, k), " no schur_keep")
    assert solver.n_backward_refactorizations == k                       # no factor is kept: a factorization per row


def test_backward_after_the_factor_has_moved_on():
    """Another solve on the handle between forward and backward: the backward pass factors once, then solves all rows on that."""
    name = "chain3_n90"
    lam, eta, W = _problem(name, K)
    other = load_golden("chain6_n60")[0]
    solver = CLinearSolver_HIP()
    values = torch.tensor(lam.values, device="cuda", requires_grad=True)
    eta_dev = eta.cuda().requires_grad_(True)
    X = solve_multi(solver, lam, values, eta_dev)
    assert solver.Solve_PosDef_Blocky(other, other.rhs.copy())           # (another structure, too)
    (W.cuda() * X).sum().backward()
    assert solver.n_backward_refactorizations == 1
    _assert_matches_dense(name, K, (X.detach(), values.grad, eta_dev.grad), " (factor taken away)")
    # the handle's factor is this node's again: a second backward pass would not factor (generation rule)
    X2 = solve_multi(solver, lam, values, eta_dev)
    (W.cuda() * X2).sum().backward()
    assert solver.n_backward_refactorizations == 1


def test_only_eta_needs_a_gradient(monkeypatch):
    name = "chain6_n60"
    lam, eta, W = _problem(name, K)
    solver = CLinearSolver_HIP()
    monkeypatch.setattr(solver, "pattern_outer_sum_device", lambda *args: pytest.fail("the outer-product kernel was launched"))
    values = torch.tensor(lam.values, device="cuda")
    eta_dev = eta.cuda().requires_grad_(True)
    X = solve_multi(solver, lam, values, eta_dev)
    (W.cuda() * X).sum().backward()
    assert values.grad is None and rel_inf(eta_dev.grad, _dense_reference(name, K)[2]) < TOL


def test_not_positive_definite_raises():
    lam = load_golden("indefinite_n40")[0]
    solver = CLinearSolver_HIP()
    values = torch.tensor(lam.values, device="cuda", requires_grad=True)
    eta = torch.tensor(lam.rhs, device="cuda").repeat(3, 1).requires_grad_(True)
    with pytest.raises(torch.linalg.LinAlgError):
        solve_multi(solver, lam, values, eta)
    assert values.grad is None and eta.grad is None
    _assert_matches_dense("chain6_n60", K, _device_gradients(solver, "chain6_n60", K), " after a refused matrix")


def test_wrong_arguments_raise_before_any_library_call():
    lam = load_golden("chain6_n60")[0]
    n = lam.n_scalars
    solver = CLinearSolver_HIP()
    values = torch.tensor(lam.values, device="cuda")
    eta = torch.tensor(lam.rhs, device="cuda").repeat(2, 1)
    overlapping = torch.zeros(2 * n, dtype=torch.float64, device="cuda").as_strided((2, n), (n - 1, 1))
    for bad_values, bad_eta, error in [(values.float(), eta, TypeError), (values, eta.float(), TypeError),
                                       (values.cpu(), eta, ValueError), (values, eta.cpu(), ValueError),
                                       (values[:-1], eta, ValueError), (values, eta[0], ValueError),
                                       (values, eta[:, :-1], ValueError), (values, eta[None], ValueError),
                                       (values, eta[:0], ValueError), (values, eta[:1].repeat(MAX_COLUMNS + 1, 1), ValueError),
                                       (values, eta.T.contiguous().T, ValueError), (values, overlapping, ValueError),
                                       (values, lam.rhs[None, :], TypeError), (lam.values, eta, TypeError)]:
        with pytest.raises(error):
            solve_multi(solver, lam, bad_values, bad_eta)
    with pytest.raises(TypeError):
        solve_multi(object(), lam, values, eta)
    assert solver.factor_generation == 0 and not solver._analyzed and solver._structure_key is None
