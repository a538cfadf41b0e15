"""The differentiable solve (slam_plus_plus_amd/torch_solve.py) on the device, in both modes: the forward solution bit for bit
against slampp_hip_factor_solve_device, both gradients of loss = w^T x against fp64 dense autograd on the CPU
(dense_from_packed + torch.linalg.solve) to the project's parity tolerance of 1e-10 rel-inf, who owns the kept factor, the
chain rule through torch ops on the current and on a side stream, matrices that are not positive definite, batches, and
the argument checks."""
import functools

import numpy as np
import pytest
import torch

from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP, CLinearSolver_Schur_HIP
from slam_plus_plus_amd.torch_solve import solve, solve_batch, dense_from_packed, _element_rows_cols
from golden_util import load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-10
SPARSE = ["chain3_n90", "chain6_n60", "chain7_n40", "manhattan_n150", "sphere_8x8"]
BA = ["ba_12x150_venice", "ba_10x120_band"]


def rel_inf(got, ref):
    got, ref = got.detach().cpu().numpy(), ref.detach().cpu().numpy()
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def _w(n, seed=31):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(n))


@functools.lru_cache(maxsize=None)
def _dense_reference(name):
    """(x, values gradient, eta gradient) of loss = w^T M(values)^-1 eta by dense autograd on the CPU; computed once."""
    lam = load_golden(name)[0]
    values = torch.from_numpy(lam.values).clone().requires_grad_(True)
    eta = torch.from_numpy(lam.rhs).clone().requires_grad_(True)
    x = torch.linalg.solve(dense_from_packed(lam, values), eta)
    (_w(lam.n_scalars) @ x).backward()
    return x.detach(), values.grad, eta.grad


def _device_gradients(solver, lam):
    values = torch.tensor(lam.values, device="cuda", requires_grad=True)
    eta = torch.tensor(lam.rhs, device="cuda", requires_grad=True)
    x = solve(solver, lam, values, eta)
    (_w(lam.n_scalars).cuda() @ x).backward()
    return x.detach(), values.grad, eta.grad


def _assert_matches_dense(name, got, what=""):
    ref = _dense_reference(name)
    errs = [rel_inf(g, r) for g, r in zip(got, ref)]
    print(f"{name}{what}: rel-inf of x {errs[0]:.2e}, of the values gradient {errs[1]:.2e}, of the eta gradient {errs[2]:.2e}")
    assert max(errs) < TOL


def _assert_forward_bits(make_solver, lam, x):
    plain = make_solver()
    plain.SymbolicDecomposition_Blocky(lam)
    vals, rhs = torch.tensor(lam.values, device="cuda"), torch.tensor(lam.rhs, device="cuda")
    assert plain.factor_solve_device(vals.data_ptr(), rhs.data_ptr())
    assert torch.equal(x, rhs)


@pytest.mark.parametrize("name", SPARSE)
def test_sparse_mode_forward_and_gradients(name):
    lam = load_golden(name)[0]
    solver = CLinearSolver_HIP()
    got = _device_gradients(solver, lam)
    _assert_forward_bits(CLinearSolver_HIP, lam, got[0])
    _assert_matches_dense(name, got)
    assert solver.n_backward_refactorizations == 0                       # two substitutions on the kept factor


@pytest.mark.parametrize("name", BA)
@pytest.mark.parametrize("schur_sparse", [0, 1])
def test_schur_mode_with_the_kept_factor(name, schur_sparse):
    lam = load_golden(name)[0]

    def make():
        return CLinearSolver_Schur_HIP(schur_keep=1, schur_sparse=schur_sparse)
    solver = make()
    got = _device_gradients(solver, lam)
    _assert_forward_bits(make, lam, got[0])
    _assert_matches_dense(name, got, f" schur_sparse={schur_sparse}")
    assert solver.n_backward_refactorizations == 0


@pytest.mark.parametrize("name", BA)
def test_schur_mode_without_schur_keep_factors_again(name):
    lam = load_golden(name)[0]
    solver = CLinearSolver_Schur_HIP()
    _assert_matches_dense(name, _device_gradients(solver, lam), " no schur_keep")
    assert solver.n_backward_refactorizations == 1


def test_backward_of_an_earlier_forward_factors_again():
    """Two forwards on one handle (two structures), then backward of the first and of the second."""
    lam1, lam2 = load_golden("chain6_n60")[0], load_golden("manhattan_n150")[0]
    solver = CLinearSolver_HIP()
    leaves, xs = [], []
    for lam in (lam1, lam2):
        values = torch.tensor(lam.values, device="cuda", requires_grad=True)
        eta = torch.tensor(lam.rhs, device="cuda", requires_grad=True)
        leaves.append((values, eta))
        xs.append(solve(solver, lam, values, eta))
    (_w(lam1.n_scalars).cuda() @ xs[0]).backward()
    assert solver.n_backward_refactorizations == 1                       # the factor was the second forward's
    _assert_matches_dense("chain6_n60", (xs[0], leaves[0][0].grad, leaves[0][1].grad), " (first of two)")
    (_w(lam2.n_scalars).cuda() @ xs[1]).backward()
    assert solver.n_backward_refactorizations == 2                       # ... and now it is the first one's again
    _assert_matches_dense("manhattan_n150", (xs[1], leaves[1][0].grad, leaves[1][1].grad), " (second of two)")
    # a factorizing call through the wrapper, a product on another structure and Free_Memory take the factor away too
    for n_expected, steal in enumerate([lambda: solver.Solve_PosDef_Blocky(lam1, lam1.rhs.copy()),
                                        lambda: solver.Multiply(lam2, lam2.rhs.copy()), solver.Free_Memory], 3):
        values = torch.tensor(lam1.values, device="cuda", requires_grad=True)
        eta = torch.tensor(lam1.rhs, device="cuda", requires_grad=True)
        x = solve(solver, lam1, values, eta)
        steal()
        (_w(lam1.n_scalars).cuda() @ x).backward()
        assert solver.n_backward_refactorizations == n_expected
        _assert_matches_dense("chain6_n60", (x, values.grad, eta.grad), f" (factor taken away, {n_expected - 2})")


def test_only_eta_needs_a_gradient(monkeypatch):
    lam = load_golden("chain6_n60")[0]
    solver = CLinearSolver_HIP()
    monkeypatch.setattr(solver, "pattern_outer_device", lambda *args: pytest.fail("the outer-product kernel was launched"))
    values = torch.tensor(lam.values, device="cuda")
    eta = torch.tensor(lam.rhs, device="cuda", requires_grad=True)
    x = solve(solver, lam, values, eta)
    (_w(lam.n_scalars).cuda() @ x).backward()
    assert values.grad is None and rel_inf(eta.grad, _dense_reference("chain6_n60")[2]) < TOL


def _damping_direction(lam):
    """The packed values of mean(diag M) * I: the direction Levenberg-Marquardt damps along."""
    row, col, _ = _element_rows_cols(lam)
    return (row == col) * float(lam.values[row == col].mean())


@functools.lru_cache(maxsize=None)
def _dense_theta_reference(name, f_theta):
    lam = load_golden(name)[0]
    theta = torch.tensor(f_theta, dtype=torch.float64, requires_grad=True)
    values = torch.from_numpy(lam.values) + theta * torch.from_numpy(_damping_direction(lam))
    x = torch.linalg.solve(dense_from_packed(lam, values), torch.from_numpy(lam.rhs))
    (_w(lam.n_scalars) @ x).backward()
    return float(theta.grad)


@pytest.mark.parametrize("side_stream", [False, True])
@pytest.mark.parametrize("name,schur", [("sphere_8x8", False), ("ba_12x150_venice", True)])
def test_chain_rule_through_torch(name, schur, side_stream):
    """values = base + theta * direction with a scalar leaf theta, the values made by a torch op enqueued right before the
    call -- on torch's current stream or on a side stream, which the solver's stream has to wait for."""
    lam = load_golden(name)[0]
    solver = CLinearSolver_Schur_HIP(schur_keep=1) if schur else CLinearSolver_HIP()
    base, direction = torch.tensor(lam.values, device="cuda"), torch.tensor(_damping_direction(lam), device="cuda")
    eta, w = torch.tensor(lam.rhs, device="cuda"), _w(lam.n_scalars).cuda()
    theta = torch.tensor(0.3, dtype=torch.float64, device="cuda", requires_grad=True)
    solver.SymbolicDecomposition_Blocky(lam)                             # (the host work is not what this test is about)
    stream = torch.cuda.Stream() if side_stream else torch.cuda.current_stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        values = base + theta * direction
        loss = w @ solve(solver, lam, values, eta)
        loss.backward()
    stream.synchronize()
    ref = _dense_theta_reference(name, 0.3)
    err = abs(float(theta.grad) - ref) / abs(ref)
    print(f"{name} side_stream={side_stream}: d loss / d theta {float(theta.grad):.15e}, dense {ref:.15e}, relative {err:.2e}")
    assert err < TOL and solver.n_backward_refactorizations == 0


def test_not_positive_definite_raises():
    lam = load_golden("indefinite_n40")[0]
    solver = CLinearSolver_HIP()
    values = torch.tensor(lam.values, device="cuda", requires_grad=True)
    eta = torch.tensor(lam.rhs, device="cuda", requires_grad=True)
    with pytest.raises(torch.linalg.LinAlgError):
        solve(solver, lam, values, eta)
    assert values.grad is None and eta.grad is None
    good = load_golden("chain6_n60")[0]                                  # the handle still answers
    _assert_matches_dense("chain6_n60", _device_gradients(solver, good), " after a refused matrix")


@functools.lru_cache(maxsize=None)
def _dense_batch_reference(name, dampings):
    lam = load_golden(name)[0]
    direction = torch.from_numpy(_damping_direction(lam))
    out = []
    for k, f_damping in enumerate(dampings):
        values = (torch.from_numpy(lam.values) + f_damping * direction).requires_grad_(True)
        eta = (torch.from_numpy(lam.rhs) * (k + 1)).requires_grad_(True)
        x = torch.linalg.solve(dense_from_packed(lam, values), eta)
        (_w(lam.n_scalars, 40 + k) @ x).backward()
        out.append((x.detach(), values.grad, eta.grad))
    return [torch.stack(t) for t in zip(*out)]


@pytest.mark.parametrize("values_pad", [0, 1], ids=["shared_launches", "member_by_member"])
def test_batch_of_three_damped_copies(values_pad):
    """K = 3 damping values of chain6_n60 (an even number of values); a row stride of n_values + 1 is odd, which the library
    solves member by member."""
    name, dampings = "chain6_n60", (0.0, 0.1, 1.0)
    lam = load_golden(name)[0]
    n_values, n = lam.values.shape[0], lam.n_scalars
    assert n_values % 2 == 0
    direction = torch.tensor(_damping_direction(lam), device="cuda")
    buf = torch.zeros((3, n_values + values_pad), dtype=torch.float64, device="cuda")
    buf[:, :n_values] = torch.tensor(lam.values, device="cuda") + torch.tensor(dampings, dtype=torch.float64, device="cuda")[:, None] * direction
    values = buf[:, :n_values].detach().requires_grad_(True)
    assert values.stride(0) % 2 == values_pad
    eta = (torch.tensor(lam.rhs, device="cuda") * torch.arange(1, 4, device="cuda")[:, None]).requires_grad_(True)
    w = torch.stack([_w(n, 40 + k) for k in range(3)]).cuda()
    solver = CLinearSolver_HIP()
    x = solve_batch(solver, lam, values, eta)
    (w * x).sum().backward()
    ref = _dense_batch_reference(name, dampings)
    errs = [rel_inf(g, r) for g, r in zip((x, values.grad, eta.grad), ref)]
    print(f"batch ({'odd' if values_pad else 'even'} stride): rel-inf of x {errs[0]:.2e}, values gradient {errs[1]:.2e}, eta gradient {errs[2]:.2e}")
    assert max(errs) < TOL and values.grad.shape == values.shape


def test_batch_names_the_member_that_is_not_positive_definite():
    lam = load_golden("chain6_n60")[0]
    values = torch.tensor(lam.values, device="cuda").repeat(3, 1)
    values[1] -= 1e3 * torch.tensor(_damping_direction(lam), device="cuda")
    eta = torch.tensor(lam.rhs, device="cuda").repeat(3, 1)
    with pytest.raises(torch.linalg.LinAlgError, match=r"\[1\]"):
        solve_batch(CLinearSolver_HIP(), lam, values, eta)


def test_wrong_arguments_raise_before_any_library_call():
    lam = load_golden("chain6_n60")[0]
    solver = CLinearSolver_HIP()
    values, eta = torch.tensor(lam.values, device="cuda"), torch.tensor(lam.rhs, device="cuda")
    strided = torch.zeros(2 * lam.n_scalars, dtype=torch.float64, device="cuda")[::2]
    for bad_values, bad_eta, error in [(values.float(), eta, TypeError), (values, eta.float(), TypeError),
                                       (values.cpu(), eta, ValueError), (values, eta.cpu(), ValueError),
                                       (values[:-1], eta, ValueError), (values, eta[None, :], ValueError),
                                       (values, strided, ValueError), (lam.values, eta, TypeError)]:
        with pytest.raises(error):
            solve(solver, lam, bad_values, bad_eta)
    with pytest.raises(TypeError):
        solve(object(), lam, values, eta)
    with pytest.raises(TypeError):
        solve_batch(CLinearSolver_Schur_HIP(), lam, values[None, :], eta[None, :])       # sparse mode only
    with pytest.raises(ValueError):
        solve_batch(solver, lam, values, eta)                                            # not (K, n_values)
    with pytest.raises(TypeError):
        solve_batch(solver, lam, values[None, :].float(), eta[None, :])
    assert solver.factor_generation == 0 and not solver._analyzed and solver._structure_key is None
