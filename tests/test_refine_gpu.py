"""Iterative refinement with the kept factor (slampp_hip_refine) on the conditioning sweep (tests/golden/cond_*.npz): the
chains through the sparse block path, the BA systems through the Schur path with the option schur_keep.

The yardstick is the normwise backward error  omega(x) = |eta - Lambda x|_inf / (|Lambda|_inf |x|_inf + |eta|_inf),
computed on the host from the fixture's values: two steps must not make it worse, must bring it to within a small factor of
what the best of the reference's own five solvers reaches on the same system, and must leave the forward-error bounds of
the conditioning tests standing.  (The residual is plain fp64: a smaller forward error is not promised.)

Measured on one MI355X (2026-10-17) with every step applied, before a step that does not at least halve the device's
residual norm was taken back (omega unrefined -> after two plain steps, the reference's best); DESIGN.md 4.4 says what the
rule changes:
    cond_ba_1e12         3.49e-17 -> 5.75e-20   5.43e-20
    cond_ba_1e6          1.40e-17 -> 2.48e-18   2.02e-18
    cond_ba_1e9          6.31e-20 -> 6.78e-20   3.67e-20      (device norms 4.25e-10, 1.73e-10, 4.15e-10: the second step is taken back)
    cond_ba_lm_200cams   1.59e-17 -> 1.29e-17   1.06e-17
    cond_chain3_1e7      1.96e-17 -> 1.87e-17   1.03e-17
    cond_chain6_1e12     6.22e-18 -> 5.02e-18   4.94e-18
    cond_chain6_1e6      3.33e-17 -> 7.29e-18   1.27e-17
    cond_chain6_1e9      7.45e-18 -> 5.71e-18   3.13e-18
"""
import numpy as np
import pytest

from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP, CLinearSolver_Schur_HIP
from golden_util import cond_names, load_cond, cond_bounds, rel_inf

pytestmark = pytest.mark.gpu

PD = [n for n in cond_names() if bool(load_cond(n)[1]["positive_definite"])]
MARGIN = 4.0         # over the reference's best solver: the residual is summed in another order


def _omega(A, norm_A, lam, x):
    return float(np.abs(lam.rhs - A @ x).max() / (norm_A * np.abs(x).max() + np.abs(lam.rhs).max()))


def _solver_for(lam):
    return CLinearSolver_Schur_HIP(schur_keep=1) if lam.n_matrix_cut else CLinearSolver_HIP()


@pytest.mark.parametrize("name", PD)
def test_two_steps_of_refinement(name):
    lam, ref = load_cond(name)
    A = lam.to_scipy()
    norm_A = float(abs(A).sum(axis=1).max())
    solver = _solver_for(lam)
    x0 = lam.rhs.copy()
    assert solver.Solve_PosDef(lam, x0)
    x = x0.copy()
    resid = solver.Refine(lam, lam.rhs, x, n_steps=2)
    w0, w = _omega(A, norm_A, lam, x0), _omega(A, norm_A, lam, x)
    refs = {k[2:]: _omega(A, norm_A, lam, ref[k]) for k in ref if k.startswith("x_") and k != "x_true" and bool(ref.get("ok_" + k[2:], False))}
    best = min(refs.values())
    print(f"{name}: omega unrefined {w0:.2e} -> refined {w:.2e}; reference's best {best:.2e} "
          f"({min(refs, key=refs.get)}); ratio refined / best {w / best:.2f}; residual norms {resid}")
    assert w <= w0 * (1 + 1e-3)                                          # (a)
    assert w <= MARGIN * best                                            # (b)
    b_ref, b_true = cond_bounds(ref)                                     # (c)
    x_parity = ref["x_schur"] if lam.n_matrix_cut else ref["x_cholmod_super"]
    assert rel_inf(x, x_parity) < b_ref and rel_inf(x, ref["x_true"]) < b_true
    # (d) the returned norms are |eta - Lambda x_k|_inf of the iterates, recomputed through the device product
    x1 = x0.copy()
    resid1 = solver.Refine(lam, lam.rhs, x1, n_steps=1)
    assert resid1[0] == resid[0] and resid1[1] == resid[1]               # (the same steps give the same bits)
    for k, xk in enumerate((x0, x1, x)):
        r = lam.rhs.copy()
        solver.Multiply(lam, xk, r, alpha=-1.0, beta=1.0)
        assert abs(resid[k] - np.abs(r).max()) <= 1e-12 * np.abs(r).max()


@pytest.mark.parametrize("name", PD)
def test_a_step_that_does_not_halve_the_residual_is_taken_back(name):
    """Eight steps: the reported norms never grow, every step that stands at least halves them, the first one that does
    not ends the refinement, and x is, bit for bit, the x of the steps that stood."""
    lam, _ = load_cond(name)
    solver = _solver_for(lam)
    x0 = lam.rhs.copy()
    assert solver.Solve_PosDef(lam, x0)
    x = x0.copy()
    resid = solver.Refine(lam, lam.rhs, x, n_steps=8)
    print(f"{name}: residual norms {resid}")
    n_stood = 0
    while n_stood < 8 and resid[n_stood + 1] != resid[n_stood]:
        assert 2 * resid[n_stood + 1] <= resid[n_stood]
        n_stood += 1
    assert np.all(resid[n_stood:] == resid[n_stood])
    x_stood = x0.copy()
    if n_stood:
        resid_stood = solver.Refine(lam, lam.rhs, x_stood, n_steps=n_stood)
        assert np.array_equal(resid_stood, resid[:n_stood + 1])
    assert np.array_equal(x, x_stood)
    r = lam.rhs.copy()
    solver.Multiply(lam, x, r, alpha=-1.0, beta=1.0)
    assert abs(resid[-1] - np.abs(r).max()) <= 1e-12 * np.abs(r).max()


def test_refine_needs_a_kept_factor():
    lam, _ = load_cond(PD[0])
    solver = CLinearSolver_HIP()
    solver.SymbolicDecomposition_Blocky(lam)
    with pytest.raises(ValueError):
        solver.Refine(lam, lam.rhs, lam.rhs.copy(), n_steps=1)
    ba = [n for n in PD if load_cond(n)[0].n_matrix_cut][0]
    lam, _ = load_cond(ba)
    solver = CLinearSolver_Schur_HIP()                                   # no schur_keep: nothing to refine with
    x = lam.rhs.copy()
    assert solver.Solve_PosDef(lam, x)
    with pytest.raises(ValueError, match="schur_keep"):
        solver.Refine(lam, lam.rhs, x, n_steps=1)


@pytest.mark.parametrize("n_steps", [0, 9])
def test_refine_takes_one_to_eight_steps(n_steps):
    lam, _ = load_cond(PD[0])
    solver = _solver_for(lam)
    x = lam.rhs.copy()
    assert solver.Solve_PosDef(lam, x)
    with pytest.raises(ValueError):
        solver.Refine(lam, lam.rhs, x, n_steps=n_steps)
