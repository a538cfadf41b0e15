"""k right-hand sides with the kept factor in one call (slampp_hip_solve_columns / slampp_hip_solve_columns_device_async), in
both modes.

Every column of a k-column call is held against three things at the project's 1e-10: the golden x_cholmod_super (column 0,
which is the fixture's eta; the mixed-dimension system has no golden and takes variant_util.refined_solution), the same
vector through slampp_hip_solve_again_device_async, and its own residual eta - Lambda x through the device product, relative
to max |eta| as tests/test_resolve_gpu.py measures it.  k runs over 1, 3, 10, 11, 48, 49, 130: on either side of the ten
right-hand sides a wave carries at 6 x 6 blocks and of the 48 columns of a pass, and three passes.  Both a packed array
(n_ld = n_scalars) and one with five doubles of padding behind every column, which must come back untouched.

Bits: the same call twice; column c of an 11-column call against the same vector solved alone (no dense top); a column of
NaN beside ten clean ones.  Where the call has no k-column kernels -- a block column of dimension 12, Schur mode -- it must
give slampp_hip_solve_again_device_async's bits.

One handle and one factorization per test; the references of a system are computed once.  Every test prints its worst figures."""
import functools

import numpy as np
import pytest

from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP, CLinearSolver_Schur_HIP, SOLVE_MAX_COLUMNS
from golden_util import load_golden, rel_inf
from variant_util import PLAN_OPTIONS, MIXED_SEED

pytestmark = pytest.mark.gpu

TOL = 1e-10                        # the project's bound
KS = (1, 3, 10, 11, 48, 49, 130)
K_MAX = max(KS)
PAD = 5
SENTINEL = -777.25
SYSTEMS = ["chain3_n90", "chain6_n60", "chain7_n40", "manhattan_n150", "sphere_8x8", "mixed"]
OPTIONS = {"default": {}, "many_stages": PLAN_OPTIONS, "natural_order": {"natural_order": 1},
           "dense_top": {"dense_top_nb": 2, "dense_top_min_dim": 0}}
SCHUR_GOLDENS = ["ba_10x120_band", "ba_12x150_venice"]


@functools.lru_cache(maxsize=None)
def system(name):
    """(the system, the reference solution of its own eta, the K_MAX right-hand sides: row 0 eta, the others seeded normals)"""
    if name == "mixed":
        from test_sparse_gpu import random_system
        from variant_util import refined_solution
        lam, _ = random_system(MIXED_SEED)
        dims = np.diff(lam.cumsum)
        assert len(set(dims.tolist())) > 1 and int(dims.max()) <= 8
        x_ref = refined_solution(lam)
    elif name == "wide12":
        from test_logdet_gpu import wide_system
        lam = wide_system((12, 3))
        assert int(np.diff(lam.cumsum).max()) == 12
        x_ref = np.linalg.solve(lam.to_scipy().toarray(), lam.rhs)
    else:
        lam, ref = load_golden(name)
        x_ref = ref["x_schur"] if lam.n_matrix_cut else ref["x_cholmod_super"]
    B = np.random.default_rng(20240 + len(name)).standard_normal((K_MAX, lam.n_scalars))
    B[0] = lam.rhs
    B.setflags(write=False)
    return lam, x_ref, B


def _dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def solve_columns(solver, B, ld):
    """The device call on a copy of B's rows at the leading dimension ld: (solutions, what stands in the padding)."""
    import torch
    k, n = B.shape
    buf = torch.full((k, ld), SENTINEL, dtype=torch.float64, device="cuda")
    buf[:, :n] = torch.from_numpy(np.ascontiguousarray(B)).cuda()
    torch.cuda.synchronize()                                             # (torch fills on its own stream, the library reads on the handle's)
    generation = solver.factor_generation
    solver.solve_columns_device(buf.data_ptr(), ld, k)
    assert solver.sync() and solver.factor_generation == generation      # (it installs no factor)
    out = buf.cpu().numpy()
    return out[:, :n].copy(), out[:, n:].copy()


def solve_again_rows(solver, B):
    """Every row of B through slampp_hip_solve_again_device_async."""
    X = _dev(B)
    for c in range(B.shape[0]):
        solver.solve_again_device(X.data_ptr() + 8 * c * B.shape[1])
    assert solver.sync()
    return X.cpu().numpy()


def worst_residual(solver, vals, B, X):
    """max over the columns of max |eta - Lambda x| / max |eta|, through the device product."""
    R, Xd = _dev(B), _dev(X)
    n = B.shape[1]
    for c in range(B.shape[0]):
        solver.multiply_device(vals.data_ptr(), Xd.data_ptr() + 8 * c * n, R.data_ptr() + 8 * c * n, -1.0, 1.0)
    assert solver.sync()
    return float((np.abs(R.cpu().numpy()).max(axis=1) / np.abs(B).max(axis=1)).max())


def worst_rel_inf(X, ref):
    return max(rel_inf(X[c], ref[c]) for c in range(X.shape[0]))


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def factored_sparse_solver(lam, options):
    solver = CLinearSolver_HIP(**options)
    solver.SymbolicDecomposition_Blocky(lam)
    vals, eta = _dev(lam.values), _dev(lam.rhs)
    assert solver.factor_solve_device(vals.data_ptr(), eta.data_ptr())
    return solver, vals, eta.cpu().numpy()


# ---- sparse mode: the k-column kernels ----

@pytest.mark.parametrize("variant", list(OPTIONS))
@pytest.mark.parametrize("name", SYSTEMS)
def test_sparse_columns(name, variant):
    lam, x_ref, B = system(name)
    n = lam.n_scalars
    solver, vals, x_first = factored_sparse_solver(lam, OPTIONS[variant])
    assert rel_inf(x_first, x_ref) < TOL
    plan = solver.plan()
    assert (plan["dense_dim"] > 0) == (variant == "dense_top")
    X_again = solve_again_rows(solver, B)
    worst = {"reference": 0.0, "solve_again": 0.0, "residual": 0.0}
    for k in KS:
        for ld in (n, n + PAD):
            X, pad = solve_columns(solver, B[:k], ld)
            assert np.all(pad == SENTINEL), (k, ld)
            figures = {"reference": rel_inf(X[0], x_ref), "solve_again": worst_rel_inf(X, X_again[:k]),
                       "residual": worst_residual(solver, vals, B[:k], X)}
            for what, f in figures.items():
                worst[what] = max(worst[what], f)
            again, _ = solve_columns(solver, B[:k], ld)
            assert same_bits(X, again), (k, ld)                         # the same call twice
            assert all(f < TOL for f in figures.values()), (k, ld, figures)
    print(f"solve_columns {name} [{variant}]: worst rel_inf against the reference {worst['reference']:.2e}, against "
          f"solve_again {worst['solve_again']:.2e}, worst residual {worst['residual']:.2e}")
    # a column of NaN reaches no other column
    clean, _ = solve_columns(solver, B[:11], n)
    dirty_B = B[:11].copy()
    dirty_B[4] = np.nan
    dirty, _ = solve_columns(solver, dirty_B, n)
    others = [c for c in range(11) if c != 4]
    assert np.all(np.isnan(dirty[4])) and np.all(np.isfinite(dirty[others]))
    assert same_bits(dirty[others], clean[others])
    after, _ = solve_columns(solver, B[:11], n)                          # and nothing of it stays behind
    assert same_bits(after, clean)
    if variant == "many_stages":                                         # (no dense top) a column does not depend on its company
        for c in range(11):
            alone, _ = solve_columns(solver, B[c:c + 1], n)
            assert same_bits(alone[0], clean[c]), c
    # the handle is left as it was: the single-vector route gives what it gave
    assert same_bits(solve_again_rows(solver, B[:2]), X_again[:2])


def test_block_column_of_dimension_12_takes_the_single_vector_route():
    lam, x_ref, B = system("wide12")
    n = lam.n_scalars
    solver, vals, x_first = factored_sparse_solver(lam, {"natural_order": 1})
    assert rel_inf(x_first, x_ref) < TOL
    X_again = solve_again_rows(solver, B[:11])
    for ld in (n, n + PAD):
        X, pad = solve_columns(solver, B[:11], ld)
        assert np.all(pad == SENTINEL) and same_bits(X, X_again)
    resid = worst_residual(solver, vals, B[:11], X)
    print(f"solve_columns wide12: rel_inf against the reference {rel_inf(X[0], x_ref):.2e}, worst residual {resid:.2e}")
    assert rel_inf(X[0], x_ref) < TOL and resid < TOL


# ---- Schur mode: the single-vector route, column by column ----

def check_schur_columns(solver, lam, x_ref, B, what):
    n = lam.n_scalars
    X_again = solve_again_rows(solver, B[:11])
    for ld in (n, n + PAD):
        X, pad = solve_columns(solver, B[:11], ld)
        assert np.all(pad == SENTINEL) and same_bits(X, X_again), (what, ld)
    print(f"solve_columns {what}: rel_inf against x_schur {rel_inf(X[0], x_ref):.2e}")
    assert rel_inf(X[0], x_ref) < TOL


@pytest.mark.parametrize("sparse", [0, 1])
@pytest.mark.parametrize("name", SCHUR_GOLDENS)
def test_schur_columns_with_schur_keep(name, sparse):
    lam, x_ref, B = system(name)
    solver = CLinearSolver_Schur_HIP(schur_keep=1, schur_sparse=sparse)
    eta = lam.rhs.copy()
    assert solver.Solve_PosDef(lam, eta) and rel_inf(eta, x_ref) < TOL
    check_schur_columns(solver, lam, x_ref, B, f"{name} [schur_keep, schur_sparse={sparse}]")


@pytest.mark.parametrize("sparse", [0, 1])
@pytest.mark.parametrize("name", SCHUR_GOLDENS)
def test_schur_columns_after_a_covariance_call(name, sparse):
    lam, x_ref, B = system(name)
    solver = CLinearSolver_Schur_HIP(schur_sparse=sparse)
    solver.Marginals_Pattern(lam)
    check_schur_columns(solver, lam, x_ref, B, f"{name} [after Marginals_Pattern, schur_sparse={sparse}]")


# ---- the host form ----

def test_host_form_sparse():
    lam, x_ref, B = system("chain6_n60")
    solver, _, _ = factored_sparse_solver(lam, {})
    X_dev, _ = solve_columns(solver, B[:60], lam.n_scalars)              # (60 columns: two groups through device memory)
    X = B[:60].copy()
    assert solver.Solve_Columns(X)
    assert same_bits(X, X_dev) and rel_inf(X[0], x_ref) < TOL
    with pytest.raises(ValueError):
        solver.Solve_Columns(B[:2, :-1].copy())
    with pytest.raises(ValueError):
        solver.Solve_Columns(np.zeros((SOLVE_MAX_COLUMNS + 1, lam.n_scalars)))


def test_host_form_schur():
    lam, x_ref, B = system("ba_10x120_band")
    solver = CLinearSolver_Schur_HIP(schur_keep=1)
    assert solver.Solve_PosDef(lam, lam.rhs.copy())
    X = B[:5].copy()
    assert solver.Solve_Columns(X)
    assert same_bits(X, solve_again_rows(solver, B[:5])) and rel_inf(X[0], x_ref) < TOL


# ---- refusals ----

def test_refusals():
    import torch
    lam, _, B = system("chain6_n60")
    n = lam.n_scalars
    buf = _dev(B[:3])
    solver = CLinearSolver_HIP()
    solver.SymbolicDecomposition_Blocky(lam)
    with pytest.raises(ValueError, match="solve_columns: no valid factorization"):         # nothing factored yet
        solver.solve_columns_device(buf.data_ptr(), n, 3)
    with pytest.raises(ValueError, match="solve_columns: no valid factorization"):
        solver.Solve_Columns(B[:3].copy())
    vals, eta = _dev(lam.values), _dev(lam.rhs)
    assert solver.factor_solve_device(vals.data_ptr(), eta.data_ptr())
    for k in (0, -1, SOLVE_MAX_COLUMNS + 1):
        with pytest.raises(ValueError, match="SLAMPP_HIP_SOLVE_MAX_COLUMNS"):
            solver.solve_columns_device(buf.data_ptr(), n, k)
    with pytest.raises(ValueError, match="leading dimension"):
        solver.solve_columns_device(buf.data_ptr(), n - 1, 2)
    with pytest.raises(ValueError, match="null"):
        solver.solve_columns_device(0, n, 3)
    solver.solve_columns_device(buf.data_ptr(), 0, 1)                    # one column: the leading dimension is not read
    big = torch.zeros((SOLVE_MAX_COLUMNS, n), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    solver.solve_columns_device(big.data_ptr(), n, SOLVE_MAX_COLUMNS)   # the largest call there is
    assert solver.sync() and float(big.abs().max()) == 0.0
    # a factorization that fails leaves nothing to solve from
    bad, _ = load_golden("indefinite_n40")
    failing = CLinearSolver_HIP()
    assert failing.Solve_PosDef(bad, bad.rhs.copy()) is False
    with pytest.raises(ValueError, match="solve_columns: no valid factorization"):
        failing.solve_columns_device(_dev(np.zeros((2, bad.n_scalars))).data_ptr(), bad.n_scalars, 2)


def test_schur_refusals():
    lam, _, B = system("ba_10x120_band")
    buf = _dev(B[:2])
    plain = CLinearSolver_Schur_HIP()
    assert plain.Solve_PosDef(lam, lam.rhs.copy())
    with pytest.raises(ValueError, match="solve_columns.*schur_keep"):   # no kept factor: the message names the option
        plain.solve_columns_device(buf.data_ptr(), lam.n_scalars, 2)
    with pytest.raises(ValueError, match="schur_keep"):
        plain.Solve_Columns(B[:2].copy())
    shards = CLinearSolver_Schur_HIP(devices=[0, 0], schur_keep=1)
    assert shards.Solve_PosDef(lam, lam.rhs.copy())
    with pytest.raises(NotImplementedError, match="solve_columns"):
        shards.solve_columns_device(buf.data_ptr(), lam.n_scalars, 2)
