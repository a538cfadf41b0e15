"""The differentiable log-determinant (slam_plus_plus_amd/torch_solve.py: logdet) on the device, in both modes: the value and
the gradient in the packed values against torch.logdet(dense_from_packed(lam, values)) with fp64 autograd on the CPU, to the
project's parity tolerance of 1e-10 rel-inf (as test_torch_solve_gpu.py applies it to the solve); the chain rule through torch
ops on the current and on a side stream; a matrix that is not positive definite; the argument checks; and the backward pass
where the covariance call it needs is not supported."""
import functools

import numpy as np
import pytest
import torch

from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP, CLinearSolver_Schur_HIP
from slam_plus_plus_amd.torch_solve import logdet, dense_from_packed, _element_rows_cols
from golden_util import load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-10
SPARSE = ["chain3_n90", "chain6_n60", "chain7_n40", "manhattan_n150", "sphere_8x8"]
BA = ["ba_12x150_venice", "ba_10x120_band"]


def rel_inf(got, ref):
    got, ref = got.detach().cpu().numpy(), ref.detach().cpu().numpy()
    return float(np.abs(got - ref).max() / np.abs(ref).max())


@functools.lru_cache(maxsize=None)
def _dense_reference(name):
    """(log det, its gradient in the values) by dense autograd on the CPU; computed once."""
    lam = load_golden(name)[0]
    values = torch.from_numpy(lam.values).clone().requires_grad_(True)
    y = torch.logdet(dense_from_packed(lam, values))
    y.backward()
    return y.detach(), values.grad


def _check(name, solver, what=""):
    lam = load_golden(name)[0]
    values = torch.tensor(lam.values, device="cuda", requires_grad=True)
    y = logdet(solver, lam, values)
    assert y.shape == () and y.dtype == torch.float64 and y.is_cuda
    y.backward()
    y_ref, grad_ref = _dense_reference(name)
    errs = rel_inf(y, y_ref), rel_inf(values.grad, grad_ref)
    print(f"{name}{what}: log det {float(y.detach()):.15e}, rel-inf of the value {errs[0]:.2e}, of the values gradient {errs[1]:.2e}")
    assert max(errs) < TOL
    return lam, values


@pytest.mark.parametrize("name", SPARSE)
def test_sparse_mode_value_and_gradient(name):
    _check(name, CLinearSolver_HIP())


@pytest.mark.parametrize("name", BA)
@pytest.mark.parametrize("schur_sparse", [0, 1])
def test_schur_mode_value_and_gradient(name, schur_sparse):
    _check(name, CLinearSolver_Schur_HIP(schur_sparse=schur_sparse), f" schur_sparse={schur_sparse}")


def test_weights_are_cached_per_structure():
    solver = CLinearSolver_HIP()
    lam, _ = _check("chain6_n60", solver)
    w = solver._logdet_w[1]
    _check("chain6_n60", solver, " (again)")
    assert solver._logdet_w[1] is w and w.is_cuda                        # one device tensor per structure key
    offdiag = _element_rows_cols(lam)[2]
    assert torch.equal(w.cpu(), torch.from_numpy(np.where(offdiag, 2.0, 1.0)))
    _check("sphere_8x8", solver, " (another structure on the same handle)")
    assert solver._logdet_w[1] is not w


def _scale_direction(lam):
    """log of a per-value scale: the values of the off-diagonal blocks shrink with theta^2, the diagonal blocks do not."""
    return torch.from_numpy(np.where(_element_rows_cols(lam)[2], 1.0, 0.0))


@functools.lru_cache(maxsize=None)
def _dense_theta_reference(name, f_theta):
    lam = load_golden(name)[0]
    theta = torch.tensor(f_theta, dtype=torch.float64, requires_grad=True)
    values = torch.from_numpy(lam.values) * (1 - theta ** 2 * _scale_direction(lam))
    (3 * torch.logdet(dense_from_packed(lam, values))).backward()
    return float(theta.grad)


@pytest.mark.parametrize("side_stream", [False, True])
@pytest.mark.parametrize("name,schur", [("sphere_8x8", False), ("ba_12x150_venice", True)])
def test_chain_rule_through_torch(name, schur, side_stream):
    """loss = 3 logdet(values scaled by a function of theta^2), theta a scalar leaf, the values made by torch ops enqueued
    right before the call -- on torch's current stream or on a side stream, which the solver's stream has to wait for."""
    lam = load_golden(name)[0]
    solver = CLinearSolver_Schur_HIP() if schur else CLinearSolver_HIP()
    base, direction = torch.tensor(lam.values, device="cuda"), _scale_direction(lam).cuda()
    theta = torch.tensor(0.3, dtype=torch.float64, device="cuda", requires_grad=True)
    solver.SymbolicDecomposition_Blocky(lam)                             # (the host work is not what this test is about)
    stream = torch.cuda.Stream() if side_stream else torch.cuda.current_stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        values = base * (1 - theta ** 2 * direction)
        loss = 3 * logdet(solver, lam, values)
        loss.backward()
    stream.synchronize()
    ref = _dense_theta_reference(name, 0.3)
    err = abs(float(theta.grad) - ref) / abs(ref)
    print(f"{name} side_stream={side_stream}: d loss / d theta {float(theta.grad):.15e}, dense {ref:.15e}, relative {err:.2e}")
    assert err < TOL


def test_not_positive_definite_raises():
    lam = load_golden("indefinite_n40")[0]
    solver = CLinearSolver_HIP()
    values = torch.tensor(lam.values, device="cuda", requires_grad=True)
    with pytest.raises(torch.linalg.LinAlgError):
        logdet(solver, lam, values)
    assert values.grad is None
    _check("chain6_n60", solver, " after a refused matrix")              # the handle still answers


def test_wrong_arguments_raise_before_any_library_call():
    lam = load_golden("chain6_n60")[0]
    solver = CLinearSolver_HIP()
    values = torch.tensor(lam.values, device="cuda")
    strided = torch.zeros(2 * lam.values.shape[0], dtype=torch.float64, device="cuda")[::2]
    for bad, error in [(values.float(), TypeError), (values.cpu(), ValueError), (values[:-1], ValueError),
                       (values[None, :], ValueError), (strided, ValueError), (lam.values, TypeError)]:
        with pytest.raises(error):
            logdet(solver, lam, bad)
    with pytest.raises(TypeError):
        logdet(object(), lam, values)
    assert solver.factor_generation == 0 and not solver._analyzed and solver._structure_key is None


def test_backward_names_the_limit_where_the_covariance_call_is_unsupported():
    """Block columns wider than 8: the forward pass works (they are factored in pieces), the pattern covariances do not exist."""
    from test_logdet_gpu import wide_system, dense_matrix
    lam = wide_system((11, 3))
    solver = CLinearSolver_HIP()
    values = torch.tensor(lam.values, device="cuda", requires_grad=True)
    y = logdet(solver, lam, values)
    ref = np.linalg.slogdet(dense_matrix(lam))[1]
    assert abs(float(y.detach()) - ref) < TOL * abs(ref)
    with pytest.raises(RuntimeError, match="at most 8"):
        y.backward()
