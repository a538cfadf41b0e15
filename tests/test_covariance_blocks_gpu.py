"""Covariances beyond the block diagonal (sparse mode): Lambda^-1 on Lambda's own block pattern (Marginals_Pattern) and
whole block columns of Lambda^-1 (Marginal_Columns) -- the reference's mpart_LastColumn / mpart_Column / mpart_FullMatrix
parts of CMarginals (IncrementalPolicy.h:366-372) -- against numpy's inverse and the reference's goldens."""
import numpy as np
import pytest

from slam_plus_plus_amd import synth
from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP

pytestmark = pytest.mark.gpu
TOL = 1e-10
GOLDENS = ["chain6_n60", "chain3_n90", "chain7_n40", "sphere_8x8", "manhattan_n150"]
OPTION_SETS = ({"dense_top_nb": 0}, {"dense_top_nb": 2, "dense_top_min_dim": 0}, {})   # no / a forced / the default dense top


def rel_inf(x, ref):
    return float(np.abs(x - ref).max() / np.abs(ref).max())


def block_cols(lam):
    return np.repeat(np.arange(lam.n_bcols), np.diff(lam.bcol_ptr))


def pattern_from_dense(lam, full):
    """Lambda's stored blocks of a dense matrix, in the layout of lam.values (each block column-major)."""
    cs, col = lam.cumsum, block_cols(lam)
    return np.concatenate([full[cs[r]:cs[r + 1], cs[c]:cs[c + 1]].T.ravel() for r, c in zip(lam.brow_idx, col)])


def check_pattern(lam, cov, full):
    assert cov.shape == lam.values.shape
    assert rel_inf(cov, pattern_from_dense(lam, full)) < TOL


def mixed_system(seed, n_min=30, n_max=160):
    """A random positive definite system with block sizes 2 .. 8 (a chain plus chords)."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(n_min, n_max))
    dims = rng.choice([2, 3, 6, 7, 8], size=n)
    chords = int(rng.integers(n // 2, 2 * n))
    a, b = rng.integers(0, n, chords), rng.integers(0, n, chords)
    pairs = set(zip(range(n - 1), range(1, n))) | {(min(x, y), max(x, y)) for x, y in zip(a, b) if x != y}
    cs = np.concatenate([[0], np.cumsum(dims)]).astype(np.int64)
    M = np.zeros((cs[-1], cs[-1]))
    for r, c in pairs:
        B = 0.4 * rng.standard_normal((dims[r], dims[c]))
        M[cs[r]:cs[r + 1], cs[c]:cs[c + 1]] = B
        M[cs[c]:cs[c + 1], cs[r]:cs[r + 1]] = B.T
    M += np.eye(cs[-1]) * (np.abs(M).sum(axis=1).max() * 0.6 + 1.0)
    bcol_ptr, brow, vals = [0], [], []
    for c in range(n):
        for r in range(c + 1):
            if r == c or (r, c) in pairs:
                brow.append(r)
                vals.append(M[cs[r]:cs[r + 1], cs[c]:cs[c + 1]].T.ravel())
        bcol_ptr.append(len(brow))
    lam = synth.BlockSystem(cs, np.asarray(bcol_ptr, dtype=np.int64), np.asarray(brow, dtype=np.int32), np.concatenate(vals),
                            rng.standard_normal(int(cs[-1])), 0)
    return lam, M


def columns_ref(lam, full, bcols):
    cs = lam.cumsum
    return np.concatenate([full[:, cs[c]:cs[c + 1]] for c in bcols], axis=1)


# ---- pattern ----

@pytest.mark.parametrize("name", GOLDENS)
def test_pattern_matches_goldens(name):
    from golden_util import load_golden
    lam, ref = load_golden(name)
    full = np.linalg.inv(lam.to_scipy().toarray())
    d = int(lam.cumsum[1])
    diag_at = lam.bcol_ptr[1:] - 1                                     # the diagonal block is the last of its column
    for opts in OPTION_SETS:
        solver = CLinearSolver_HIP(**opts)
        cov = solver.Marginals_Pattern(lam)
        check_pattern(lam, cov, full)
        blocks = cov.reshape(-1, d, d)[diag_at].transpose(0, 2, 1)    # column-major blocks -> [n, d, d]
        assert rel_inf(blocks, ref["cov_diag"]) < TOL, opts
        eta = lam.rhs.copy()                                           # the factor stays for another solve
        assert solver.Solve_Again(eta) and rel_inf(eta, ref["x_cholmod_super"]) < TOL, opts


@pytest.mark.parametrize("seed", range(6))
def test_pattern_mixed_block_sizes(seed):
    lam, M = mixed_system(500 + seed)
    check_pattern(lam, CLinearSolver_HIP(dense_top_nb=0).Marginals_Pattern(lam), np.linalg.inv(M))


@pytest.mark.parametrize("tiles", [0, 1])                              # the dense top factored densely / by its tile schedule
@pytest.mark.parametrize("name", ["sphere", "manhattan"])
def test_pattern_with_dense_top(name, tiles):
    """Pairs with both columns in the dense top, one of them, and neither."""
    lam = synth.sphere(24, 24) if name == "sphere" else synth.manhattan(1200)
    solver = CLinearSolver_HIP(dense_top_tiles=tiles) if name == "sphere" else \
        CLinearSolver_HIP(dense_top_nb=8, dense_top_min_dim=0, dense_top_tiles=tiles)
    cov = solver.Marginals_Pattern(lam)
    plan = solver.plan()
    assert plan["dense_dim"] > 0
    check_pattern(lam, cov, np.linalg.inv(lam.to_scipy().toarray()))


# ---- block columns ----

def test_columns_chain():
    lam = synth.pose_chain(n=300, d=6, seed=3)
    full = np.linalg.inv(lam.to_scipy().toarray())
    solver = CLinearSolver_HIP()
    n = lam.n_bcols
    for bcols in ([0], [n - 1], [137], [n - 1, 0, 57, 211, 3, 299 - 7, 150, 151, 12]):   # the last: k = 54 > one pass of 48
        X = solver.Marginal_Columns(lam, bcols)
        assert X.shape == (lam.n_scalars, 6 * len(bcols))
        assert rel_inf(X, columns_ref(lam, full, bcols)) < TOL, bcols


def test_columns_full_matrix():
    """Every column (mpart_FullMatrix), in passes, equals inv(Lambda)."""
    lam = synth.pose_chain(n=60, d=6, seed=5)
    X = CLinearSolver_HIP().Marginal_Columns(lam, np.arange(lam.n_bcols))
    assert rel_inf(X, np.linalg.inv(lam.to_scipy().toarray())) < TOL


@pytest.mark.parametrize("dense", [None, 0, 1])                       # no dense top; one factored densely / by its tile schedule
def test_columns_with_dense_top(dense):
    lam = synth.sphere(24, 24)
    solver = CLinearSolver_HIP(dense_top_nb=0) if dense is None else CLinearSolver_HIP(dense_top_tiles=dense)
    full = np.linalg.inv(lam.to_scipy().toarray())
    n = lam.n_bcols
    bcols = [n - 1, 0, n // 2, 7, n - 2, 100, 200, 300, 400]
    X = solver.Marginal_Columns(lam, bcols)
    assert (solver.plan()["dense_dim"] > 0) == (dense is not None)
    assert rel_inf(X, columns_ref(lam, full, bcols)) < TOL


@pytest.mark.parametrize("tiles", [0, 1])
def test_columns_forced_dense_top(tiles):
    lam = synth.manhattan(1200)
    full = np.linalg.inv(lam.to_scipy().toarray())
    solver = CLinearSolver_HIP(dense_top_nb=8, dense_top_min_dim=0, dense_top_tiles=tiles)
    bcols = [lam.n_bcols - 1, 3, 600]
    X = solver.Marginal_Columns(lam, bcols)
    assert solver.plan()["dense_dim"] > 0
    assert rel_inf(X, columns_ref(lam, full, bcols)) < TOL


@pytest.mark.parametrize("seed", range(4))
def test_columns_mixed_block_sizes(seed):
    lam, M = mixed_system(700 + seed)
    full = np.linalg.inv(M)
    rng = np.random.default_rng(seed)
    bcols = rng.choice(lam.n_bcols, size=min(lam.n_bcols, 12), replace=False).tolist()
    X = CLinearSolver_HIP(dense_top_nb=0).Marginal_Columns(lam, bcols)
    assert rel_inf(X, columns_ref(lam, full, bcols)) < TOL


# ---- the factor in place ----

@pytest.mark.parametrize("name", ["chain6_n60", "sphere_8x8"])
def test_factor_reuse(name):
    from golden_util import load_golden
    lam, ref = load_golden(name)
    solver = CLinearSolver_HIP()
    eta = lam.rhs.copy()
    assert solver.Solve_PosDef_Blocky(lam, eta)
    last = [lam.n_bcols - 1]
    X_reuse = solver.Marginal_Columns(lam, last, reuse_factor=True)
    X_fresh = solver.Marginal_Columns(lam, last)
    assert rel_inf(X_reuse, X_fresh) < 1e-13
    assert rel_inf(X_fresh, columns_ref(lam, np.linalg.inv(lam.to_scipy().toarray()), last)) < TOL
    eta = lam.rhs.copy()                                               # after a columns call
    assert solver.Solve_Again(eta) and rel_inf(eta, ref["x_cholmod_super"]) < TOL
    solver.Marginals_Pattern(lam)                                      # after a pattern call
    eta = lam.rhs.copy()
    assert solver.Solve_Again(eta) and rel_inf(eta, ref["x_cholmod_super"]) < TOL


# ---- full size ----

def test_full_size_c3():
    import scipy.sparse as sp
    lam = synth.pose_chain(n=100000)
    solver = CLinearSolver_HIP()
    last = lam.n_bcols - 1
    X = solver.Marginal_Columns(lam, [last])
    E = np.zeros_like(X)
    E[6 * last:6 * last + 6, :] = np.eye(6)
    A = sp.csr_matrix(lam.to_scipy())
    assert np.abs(A @ X - E).max() / np.abs(E).max() < 1e-10
    for j in (0, 5):                                                   # two scalar columns against full solves
        e = np.zeros(lam.n_scalars)
        e[6 * last + j] = 1.0
        assert solver.Solve_PosDef_Blocky(lam, e)
        assert rel_inf(X[:, j], e) < TOL
    cov = solver.Marginals_Pattern(lam)
    diag = solver.Marginals(lam)
    diag_at = lam.bcol_ptr[1:] - 1
    assert rel_inf(cov.reshape(-1, 6, 6)[diag_at].transpose(0, 2, 1), diag) < 1e-12
    rng = np.random.default_rng(11)                                    # off-diagonal pattern blocks against columns
    col = block_cols(lam)
    off = np.flatnonzero(lam.brow_idx != col)
    picks = rng.choice(off, size=20, replace=False)
    Xc = solver.Marginal_Columns(lam, sorted({int(col[k]) for k in picks}), reuse_factor=True)
    where = {c: i for i, c in enumerate(sorted({int(col[k]) for k in picks}))}
    for k in picks:
        r, c = int(lam.brow_idx[k]), int(col[k])
        blk = cov[36 * k:36 * k + 36].reshape(6, 6).T
        ref = Xc[6 * r:6 * r + 6, 6 * where[c]:6 * where[c] + 6]
        assert rel_inf(blk, ref) < TOL


# ---- refusals and failures ----

def test_refusals():
    from slam_plus_plus_amd.hip_solver import CLinearSolver_Schur_HIP
    lam = synth.pose_chain(n=40, d=6, seed=2)
    solver = CLinearSolver_HIP()
    solver.SymbolicDecomposition_Blocky(lam)
    with pytest.raises(ValueError):                                    # no factor yet
        solver.Marginal_Columns(lam, [3], reuse_factor=True)
    for bad in ([40], [-1], [3, 3], []):
        with pytest.raises(ValueError):
            solver.Marginal_Columns(lam, bad)
    ba = synth.ba(8, 200, seed=1)
    schur = CLinearSolver_Schur_HIP()
    schur.SymbolicDecomposition_Blocky(ba)
    from slam_plus_plus_amd.hip_solver import _ptr                    # (the Schur class has no such methods: the C entries refuse)
    with pytest.raises(NotImplementedError):
        vals = np.ascontiguousarray(ba.values)
        out = np.empty_like(vals)
        schur._check(schur._lib.slampp_hip_marginals_pattern(schur._h, _ptr(vals), _ptr(out)))
    with pytest.raises(NotImplementedError):
        cols = np.array([0], dtype=np.int64)
        out = np.empty(ba.n_scalars * 8)
        schur._check(schur._lib.slampp_hip_marginal_columns(schur._h, _ptr(np.ascontiguousarray(ba.values)), 1, _ptr(cols), _ptr(out)))


def test_not_positive_definite_leaves_no_factor():
    from golden_util import load_golden
    lam, _ = load_golden("indefinite_n40")
    solver = CLinearSolver_HIP()
    with pytest.raises(ArithmeticError):
        solver.Marginal_Columns(lam, [0])
    with pytest.raises(ValueError):
        solver.Marginal_Columns(lam, [0], reuse_factor=True)
    with pytest.raises(ArithmeticError):
        solver.Marginals_Pattern(lam)
    with pytest.raises(ValueError):
        solver.Marginal_Columns(lam, [1], reuse_factor=True)


# ---- repeatability ----

def test_repeatable_bitwise():
    lam = synth.sphere(24, 24)
    solver = CLinearSolver_HIP()
    bcols = [lam.n_bcols - 1, 5, 77]
    assert np.array_equal(solver.Marginal_Columns(lam, bcols), solver.Marginal_Columns(lam, bcols))
    assert np.array_equal(solver.Marginals_Pattern(lam), solver.Marginals_Pattern(lam))
