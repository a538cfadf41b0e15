"""Another right-hand side with the kept factor, device-resident, in both modes (slampp_hip_solve_again_device_async; the
host slampp_hip_solve_again in Schur mode with the option schur_keep): parity with the reference's solutions at the
project's 1e-10, the residual of a second right-hand side through the device product, and when the kept factor is and is
not valid."""
import numpy as np
import pytest

from slam_plus_plus_amd import synth
from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP, CLinearSolver_Schur_HIP
from oracle import oracle_lib as O
from golden_util import load_golden, load_cond, rel_inf

pytestmark = pytest.mark.gpu

TOL = 1e-10


def _dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def _resolve_on_device(solver, rhs):
    d = _dev(rhs)
    solver.solve_again_device(d.data_ptr())
    assert solver.sync()
    return d.cpu().numpy()


@pytest.mark.parametrize("name", ["chain6_n60", "manhattan_n150"])
def test_sparse_mode_device_resolve(name):
    lam, ref = load_golden(name)
    solver = CLinearSolver_HIP()
    solver.SymbolicDecomposition_Blocky(lam)
    with pytest.raises(ValueError):                                      # nothing factored yet
        solver.solve_again_device(_dev(lam.rhs).data_ptr())
    vals, eta = _dev(lam.values), _dev(lam.rhs)
    assert solver.factor_solve_device(vals.data_ptr(), eta.data_ptr())
    assert rel_inf(eta.cpu().numpy(), ref["x_cholmod_super"]) < TOL
    x3 = _resolve_on_device(solver, 3.0 * lam.rhs)
    assert rel_inf(x3, 3.0 * ref["x_cholmod_super"]) < TOL


def _check_schur_resolves(solver, lam, x_ref):
    """Solve_Again(-2 eta) from the host array and from device pointers, then a second, different right-hand side whose
    residual is checked through the device product."""
    eta = -2.0 * lam.rhs
    assert solver.Solve_Again(eta)
    assert rel_inf(eta, -2.0 * x_ref) < TOL
    assert rel_inf(_resolve_on_device(solver, -2.0 * lam.rhs), -2.0 * x_ref) < TOL
    eta2 = np.random.default_rng(21).standard_normal(lam.n_scalars)
    x2 = eta2.copy()
    assert solver.Solve_Again(x2)
    r = eta2.copy()
    solver.Multiply(lam, x2, r, alpha=-1.0, beta=1.0)
    resid = np.abs(r).max() / np.abs(eta2).max()
    print(f"{lam.name}: second right-hand side, residual {resid:.2e}")
    assert resid < TOL


@pytest.mark.parametrize("tiles", [0, 1])
@pytest.mark.parametrize("sparse", [0, 1])
@pytest.mark.parametrize("name", ["ba_10x120_band", "ba_12x150_venice"])
def test_schur_mode_resolve_with_schur_keep(name, sparse, tiles):
    lam, ref = load_golden(name)
    solver = CLinearSolver_Schur_HIP(schur_keep=1, schur_sparse=sparse, schur_tiles=tiles)
    eta = lam.rhs.copy()
    assert solver.Solve_PosDef(lam, eta)
    assert rel_inf(eta, ref["x_schur"]) < TOL
    _check_schur_resolves(solver, lam, ref["x_schur"])
    eta = lam.rhs.copy()                                                 # and the handle goes on solving
    assert solver.Solve_PosDef_Blocky(lam, eta) and rel_inf(eta, ref["x_schur"]) < TOL


@pytest.mark.parametrize("sparse", [0, 1])
@pytest.mark.parametrize("cam_dim,pt_dim", [(7, 3), (3, 2)])
def test_schur_mode_resolve_other_block_sizes(cam_dim, pt_dim, sparse):
    lam = synth.ba(10, 100, k=3, mode="uniform", seed=31, cam_dim=cam_dim, pt_dim=pt_dim)
    ok, x_ref, _, _ = O.solve_schur(lam)
    solver = CLinearSolver_Schur_HIP(schur_keep=1, schur_sparse=sparse)
    eta = lam.rhs.copy()
    assert ok and solver.Solve_PosDef(lam, eta)
    assert rel_inf(eta, x_ref) < TOL
    _check_schur_resolves(solver, lam, x_ref)


def test_schur_mode_without_schur_keep():
    lam, ref = load_golden("ba_10x120_band")
    solver = CLinearSolver_Schur_HIP()
    eta = lam.rhs.copy()
    assert solver.Solve_PosDef(lam, eta)
    with pytest.raises(ValueError, match="schur_keep"):                  # the device call names the option
        solver.solve_again_device(_dev(lam.rhs).data_ptr())
    with pytest.raises(NotImplementedError, match="only the sparse path keeps its factor"):
        solver.Solve_Again(lam.rhs.copy())                               # the host call answers as it always has
    eta = lam.rhs.copy()
    assert solver.Solve_PosDef_Blocky(lam, eta) and rel_inf(eta, ref["x_schur"]) < TOL


@pytest.mark.parametrize("sparse", [-1, 1])
def test_schur_covariance_calls_leave_a_factor_to_resolve_with(sparse):
    lam, ref = load_golden("ba_12x150_venice")
    solver = CLinearSolver_Schur_HIP(schur_sparse=sparse)
    solver.Marginals_Pattern(lam)
    _check_schur_resolves(solver, lam, ref["x_schur"])
    eta = lam.rhs.copy()                                                 # a plain solve ends it
    assert solver.Solve_PosDef_Blocky(lam, eta)
    with pytest.raises(ValueError, match="schur_keep"):
        solver.solve_again_device(_dev(lam.rhs).data_ptr())


def test_a_factorization_that_fails_leaves_nothing_to_resolve_with():
    good, _ = load_golden("ba_10x120_band")
    solver = CLinearSolver_Schur_HIP(schur_keep=1)
    assert solver.Solve_PosDef(good, good.rhs.copy())
    solver.solve_again_device(_dev(good.rhs).data_ptr())
    assert solver.sync()
    lam, _ = load_cond("cond_ba_1e9_indefinite")
    assert solver.Solve_PosDef(lam, lam.rhs.copy()) is False
    with pytest.raises(ValueError):
        solver.solve_again_device(_dev(lam.rhs).data_ptr())
    with pytest.raises(ValueError):
        solver.Solve_Again(lam.rhs.copy())


def test_set_structure_ends_the_kept_factor():
    lam, _ = load_golden("ba_10x120_band")
    solver = CLinearSolver_Schur_HIP(schur_keep=1)
    assert solver.Solve_PosDef(lam, lam.rhs.copy())
    solver._set_structure(lam)
    with pytest.raises(ValueError):
        solver.solve_again_device(_dev(lam.rhs).data_ptr())


def test_a_handle_over_several_devices_is_refused():
    lam, ref = load_golden("ba_10x120_band")
    solver = CLinearSolver_Schur_HIP(devices=[0, 0], schur_keep=1)
    eta = lam.rhs.copy()
    assert solver.Solve_PosDef(lam, eta) and rel_inf(eta, ref["x_schur"]) < TOL
    with pytest.raises(NotImplementedError):
        solver.solve_again_device(_dev(lam.rhs).data_ptr())
