"""quad_form, sample and whiten of slam_plus_plus_amd/torch_solve.py on the device.

quad_form: G = B M^-1 B^T against numpy (dense solve) at the project's 1e-10 relative to G's largest entry, bitwise
symmetric, and torch.autograd.gradcheck in fp64 at k = 3.  The gradcheck runs in fast mode (two directional central
differences instead of one per input: a factorization each) on values whose diagonal blocks are symmetrized by torch ops in
front of the call -- the packed values carry both triangles of a diagonal block and a Cholesky factorization reads one, so
only symmetric perturbations are perturbations of M.  Its tolerance is derived, not fitted: the forward value is held to
TOL * max|G|, the central difference divides the difference of two such values by 2 eps, and fast mode contracts the k x k
output with a unit vector u (|u|_1 <= k): the numerical derivative is off by at most k * TOL * max|G| / eps.  The analytic
gradient's own error and the O(eps^2) truncation (values of size 1 .. 1e2 moved by 1e-5) are orders below that.
sample: L_ref^T P x equals z at 1e-10 for numpy's Cholesky factor of the permuted matrix; whiten against the half-forward."""
import numpy as np
import pytest
import torch

from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP, HALF_FORWARD
from slam_plus_plus_amd.torch_solve import quad_form, sample, whiten, _element_rows_cols
from golden_util import load_golden

pytestmark = pytest.mark.gpu

TOL = 1e-10
K = 3
EPS = 1e-5


def _rows(lam, k, seed):
    return np.random.default_rng(seed).standard_normal((k, lam.n_scalars))


def _dense(lam):
    return lam.to_scipy().toarray()


def _symmetrize(lam, device):
    """values -> values with every diagonal block replaced by (D + D^T) / 2, as a torch function: index of the transposed
    element of every packed value (itself off the diagonal blocks)."""
    row, col, offdiag = _element_rows_cols(lam)
    n = int(lam.cumsum[-1])
    where = {(int(r), int(c)): i for i, (r, c, o) in enumerate(zip(row, col, offdiag)) if not o}
    partner = np.arange(row.shape[0])
    for i, (r, c, o) in enumerate(zip(row, col, offdiag)):
        if not o:
            partner[i] = where[(int(c), int(r))]
    partner = torch.from_numpy(partner).to(device)
    assert n > 0
    return lambda v: 0.5 * (v + v[partner])


@pytest.mark.parametrize("name", ["chain3_n90", "chain6_n60", "manhattan_n150"])
def test_quad_form_against_numpy(name):
    lam = load_golden(name)[0]
    solver = CLinearSolver_HIP()
    for k in (1, 3, 48):
        B = _rows(lam, k, 5 + k)
        G = quad_form(solver, lam, torch.tensor(lam.values, device="cuda"), torch.tensor(B, device="cuda"))
        ref = B @ np.linalg.solve(_dense(lam), B.T)
        err = float(np.abs(G.cpu().numpy() - ref).max() / np.abs(ref).max())
        print(f"quad_form {name} k={k}: rel error {err:.2e}")
        assert err < TOL and torch.equal(G, G.T)
    with pytest.raises(ValueError):
        quad_form(solver, lam, torch.tensor(lam.values, device="cuda"), torch.zeros((49, lam.n_scalars), dtype=torch.float64, device="cuda"))


@pytest.mark.parametrize("name", ["chain3_n90", "chain6_n60"])
def test_quad_form_gradcheck(name):
    lam = load_golden(name)[0]
    solver = CLinearSolver_HIP()
    sym = _symmetrize(lam, "cuda")
    values = torch.tensor(lam.values, device="cuda", requires_grad=True)
    B = torch.tensor(_rows(lam, K, 9), device="cuda", requires_grad=True)

    def f(v, b):
        return quad_form(solver, lam, sym(v), b)
    g_max = float(f(values, B).detach().abs().max())
    atol = K * TOL * g_max / EPS
    print(f"quad_form gradcheck {name}: max|G| {g_max:.3e}, atol {atol:.3e}")
    assert torch.autograd.gradcheck(f, (values, B), eps=EPS, atol=atol, rtol=0.0, fast_mode=True, nondet_tol=0.0)


def test_quad_form_gradients_against_dense_autograd_after_the_factor_was_replaced():
    """Both gradients of sum(C * G) against dense fp64 autograd on the CPU; the handle factors another system (and another
    structure) between forward and backward."""
    from slam_plus_plus_amd.torch_solve import dense_from_packed
    lam, other = load_golden("chain6_n60")[0], load_golden("manhattan_n150")[0]
    solver = CLinearSolver_HIP()
    Bn = _rows(lam, K, 11)
    C = torch.from_numpy(np.random.default_rng(12).standard_normal((K, K)))          # (not symmetric)
    values = torch.tensor(lam.values, device="cuda", requires_grad=True)
    B = torch.tensor(Bn, device="cuda", requires_grad=True)
    G = quad_form(solver, lam, values, B)
    generation = solver.factor_generation
    assert solver.Solve_PosDef(other, other.rhs.copy())                              # the handle's factor is someone else's now
    assert solver.factor_generation != generation
    (C.cuda() * G).sum().backward()
    v_ref = torch.from_numpy(lam.values).clone().requires_grad_(True)
    B_ref = torch.from_numpy(Bn).clone().requires_grad_(True)
    G_ref = B_ref @ torch.linalg.solve(dense_from_packed(lam, v_ref), B_ref.T)
    (C * G_ref).sum().backward()
    errs = [float((got.cpu() - ref).abs().max() / ref.abs().max()) for got, ref in
            ((G.detach(), G_ref.detach()), (values.grad, v_ref.grad), (B.grad, B_ref.grad))]
    print(f"quad_form chain6_n60 after the factor was replaced: rel-inf of G {errs[0]:.2e}, of the values gradient {errs[1]:.2e}, "
          f"of the B gradient {errs[2]:.2e}")
    assert max(errs) < TOL


def _factor_reference(lam, perm):
    idx = np.concatenate([np.arange(lam.cumsum[o], lam.cumsum[o + 1]) for o in perm])
    return idx, np.linalg.cholesky(_dense(lam)[np.ix_(idx, idx)])


@pytest.mark.parametrize("name", ["chain6_n60", "sphere_8x8"])
def test_sample_and_whiten(name):
    lam = load_golden(name)[0]
    solver = CLinearSolver_HIP()
    values = torch.tensor(lam.values, device="cuda")
    Z = _rows(lam, 5, 21)
    X = sample(solver, lam, values, torch.tensor(Z, device="cuda"))
    assert not X.requires_grad
    idx, L = _factor_reference(lam, solver.factor_structure()["perm"])
    back = (L.T @ X.cpu().numpy()[:, idx].T).T                                       # L^T P x = z
    err = float((np.abs(back - Z).max(axis=1) / np.abs(Z).max(axis=1)).max())
    print(f"sample {name}: L_ref^T P x against z {err:.2e}")
    assert err < TOL
    with pytest.raises(ValueError, match="not differentiable"):
        sample(solver, lam, values.clone().requires_grad_(True), torch.tensor(Z, device="cuda"))
    # whiten: the forward half's bits on the same factor, the permutation of the factor's structure
    B = torch.tensor(_rows(lam, 4, 22), device="cuda")
    Y, perm = whiten(solver, lam, values, B)
    assert np.array_equal(perm.numpy(), solver.factor_structure()["perm"]) and perm.dtype == torch.int64
    direct = B.clone()
    torch.cuda.synchronize()
    solver.solve_half_columns_device(direct.data_ptr(), lam.n_scalars, 4, HALF_FORWARD)
    assert solver.sync() and torch.equal(Y, direct)
    from scipy.linalg import solve_triangular
    ref = solve_triangular(L, B.cpu().numpy()[:, idx].T, lower=True).T
    assert float((np.abs(Y.cpu().numpy() - ref).max(axis=1) / np.abs(ref).max(axis=1)).max()) < TOL
    chi2 = (Y * Y).sum(dim=1).cpu().numpy()                                          # b^T M^-1 b
    ref2 = np.einsum("kn,kn->k", B.cpu().numpy(), np.linalg.solve(_dense(lam), B.cpu().numpy().T).T)
    assert float(np.abs(chi2 - ref2).max() / np.abs(ref2).max()) < TOL
    with pytest.raises(ValueError, match="not differentiable"):
        whiten(solver, lam, values.clone().requires_grad_(True), B)
