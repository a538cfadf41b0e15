"""Covariances of BA systems beyond the block diagonal (Schur mode): Lambda^-1 on Lambda's pattern (Marginals_Pattern) and
whole block columns of it (Marginal_Columns), against numpy's inverse, the reference's Schur_Marginals goldens and each other."""
import numpy as np
import pytest

from slam_plus_plus_amd import synth
from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP, CLinearSolver_Schur_HIP

pytestmark = pytest.mark.gpu
TOL = 1e-10
OPTION_SETS = ({"schur_sparse": 0}, {"schur_sparse": 1, "dense_top_nb": 0}, {"marginals_dense": 1})


def rel_inf(x, ref):
    return float(np.abs(x - ref).max() / np.abs(ref).max())


def block_cols(lam):
    return np.repeat(np.arange(lam.n_bcols), np.diff(lam.bcol_ptr))


def pattern_from_dense(lam, full):
    cs, col = lam.cumsum, block_cols(lam)
    return np.concatenate([full[cs[r]:cs[r + 1], cs[c]:cs[c + 1]].T.ravel() for r, c in zip(lam.brow_idx, col)])


def system_from_dense(M, dims, rhs, n_matrix_cut):
    cumsum = np.concatenate([[0], np.cumsum(dims)]).astype(np.int64)
    bcol_ptr, brow, vals = [0], [], []
    for c in range(len(dims)):
        for r in range(c + 1):
            blk = M[cumsum[r]:cumsum[r + 1], cumsum[c]:cumsum[c + 1]]
            if r == c or np.any(blk != 0):
                brow.append(r)
                vals.append(blk.T.ravel())
        bcol_ptr.append(len(brow))
    return synth.BlockSystem(cumsum, np.asarray(bcol_ptr, dtype=np.int64), np.asarray(brow, dtype=np.int32),
                             np.concatenate(vals), rhs, n_matrix_cut)


def with_camera_chain(lam, seed=3):
    """lam plus a camera odometry chain's J^T J: off-diagonal camera blocks in A."""
    rng = np.random.default_rng(seed)
    M = lam.to_scipy().toarray()
    cs, nc = lam.cumsum, lam.n_matrix_cut
    dc = int(cs[1] - cs[0])
    for c in range(nc - 1):
        J = 0.5 * rng.standard_normal((dc, 2 * dc))
        M[cs[c]:cs[c + 2], cs[c]:cs[c + 2]] += J.T @ J
    return system_from_dense(M, np.diff(cs), lam.rhs, nc), M


SMALL = {
    "band63": lambda: synth.ba(40, 400, k=4, mode="band", seed=1),
    "venice63": lambda: synth.ba(30, 300, mode="venice", seed=2),
    "uniform73": lambda: synth.ba(20, 200, k=4, mode="uniform", seed=3, cam_dim=7),
    "tracks32": lambda: synth.ba(40, 300, mode="tracks", seed=4, cam_dim=3, pt_dim=2),
    "band_sparse_S": lambda: synth.ba(200, 3000, k=4, mode="band", seed=3),
}


@pytest.mark.parametrize("opts", OPTION_SETS, ids=["dense", "sparse", "marginals_dense"])
@pytest.mark.parametrize("name", list(SMALL))
def test_pattern_against_numpy(name, opts):
    lam = SMALL[name]()
    full = np.linalg.inv(lam.to_scipy().toarray())
    solver = CLinearSolver_Schur_HIP(**opts)
    cov = solver.Marginals_Pattern(lam)
    assert cov.shape == lam.values.shape
    assert rel_inf(cov, pattern_from_dense(lam, full)) < TOL
    cams, pts = solver.Schur_Marginals(lam)              # the diagonal blocks agree with the block-diagonal call
    off, col = lam.block_value_offsets(), block_cols(lam)
    diag = np.flatnonzero(lam.brow_idx == col)
    nc = lam.n_matrix_cut
    blocks = [cov[off[i]:off[i + 1]] for i in diag]
    assert rel_inf(np.concatenate(blocks[:nc]), cams.reshape(-1)) < TOL
    assert rel_inf(np.concatenate(blocks[nc:]), pts.reshape(-1)) < TOL


@pytest.mark.parametrize("opts", OPTION_SETS, ids=["dense", "sparse", "marginals_dense"])
def test_camera_blocks_of_A(opts):
    lam, M = with_camera_chain(synth.ba(30, 300, k=3, mode="band", seed=8))
    col = block_cols(lam)
    nc = lam.n_matrix_cut
    assert np.count_nonzero((col < nc) & (lam.brow_idx != col)) == nc - 1
    full = np.linalg.inv(M)
    solver = CLinearSolver_Schur_HIP(**opts)
    assert rel_inf(solver.Marginals_Pattern(lam), pattern_from_dense(lam, full)) < TOL
    X = solver.Marginal_Columns(lam, [0, 5, nc + 2])
    cs = lam.cumsum
    ref = np.concatenate([full[:, cs[c]:cs[c + 1]] for c in (0, 5, nc + 2)], axis=1)
    assert rel_inf(X, ref) < TOL


@pytest.mark.parametrize("name", ["ba_12x150_venice", "ba_10x120_band"])
def test_against_reference_goldens(name):
    from golden_util import load_golden
    lam, ref = load_golden(name)
    solver = CLinearSolver_Schur_HIP()
    cov = solver.Marginals_Pattern(lam)
    off, col = lam.block_value_offsets(), block_cols(lam)
    nc = lam.n_matrix_cut
    diag = np.flatnonzero(lam.brow_idx == col)
    for j, i in enumerate(diag):
        blk = cov[off[i]:off[i + 1]]
        want = (ref["cam_cov"][j] if j < nc else ref["lm_cov"][j - nc]).reshape(-1)
        assert np.abs(blk - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
    full = np.linalg.inv(lam.to_scipy().toarray())
    assert rel_inf(cov, pattern_from_dense(lam, full)) < TOL
    cams, pts = solver.Schur_Marginals(lam)                # the block-diagonal call on the same handle
    assert rel_inf(np.concatenate([cov[off[i]:off[i + 1]] for i in diag[:nc]]), cams.reshape(-1)) < TOL
    assert rel_inf(np.concatenate([cov[off[i]:off[i + 1]] for i in diag[nc:]]), pts.reshape(-1)) < TOL


@pytest.mark.parametrize("opts", OPTION_SETS, ids=["dense", "sparse", "marginals_dense"])
def test_columns_against_numpy(opts):
    lam = synth.ba(200, 3000, k=4, mode="band", seed=3) if opts.get("schur_sparse") == 1 else \
        synth.ba(30, 300, mode="venice", seed=5)
    full = np.linalg.inv(lam.to_scipy().toarray())
    cs, nc, n = lam.cumsum, lam.n_matrix_cut, lam.n_bcols
    solver = CLinearSolver_Schur_HIP(**opts)
    for cols in ([3], [nc + 7], [nc + 1, 2, n - 1, 0], list(range(0, 10)) + [nc + 11, nc + 4] + list(range(10, 14))):
        X = solver.Marginal_Columns(lam, cols)
        ref = np.concatenate([full[:, cs[c]:cs[c + 1]] for c in cols], axis=1)
        assert X.shape == ref.shape
        assert rel_inf(X, ref) < TOL
    cov = solver.Marginals_Pattern(lam)
    X = solver.Marginal_Columns(lam, [nc + 3, 1], reuse_factor=True)
    assert rel_inf(X, np.concatenate([full[:, cs[nc + 3]:cs[nc + 4]], full[:, cs[1]:cs[2]]], axis=1)) < TOL
    assert rel_inf(solver.Marginals_Pattern(lam, reuse_factor=True), cov) < TOL
    lam2 = synth.BlockSystem(lam.cumsum, lam.bcol_ptr, lam.brow_idx, lam.values * 2.0, lam.rhs, lam.n_matrix_cut)
    eta = lam2.rhs.copy()
    assert solver.Solve_PosDef_Blocky(lam2, eta)             # an intervening solve on other values
    with pytest.raises(ValueError):
        solver.Marginal_Columns(lam, [0], reuse_factor=True)
    with pytest.raises(ValueError):
        solver.Marginals_Pattern(lam, reuse_factor=True)


def test_not_positive_definite_leaves_nothing_to_reuse():
    from golden_util import load_golden
    lam, _ = load_golden("cond_ba_1e9_indefinite")
    solver = CLinearSolver_Schur_HIP()
    with pytest.raises(ArithmeticError):
        solver.Marginals_Pattern(lam)
    with pytest.raises(ValueError):
        solver.Marginal_Columns(lam, [0], reuse_factor=True)
    with pytest.raises(ArithmeticError):
        solver.Marginal_Columns(lam, [0])
    with pytest.raises(ValueError):
        solver.Marginals_Pattern(lam, reuse_factor=True)


def test_existing_paths_unharmed():
    lam = synth.ba(40, 500, mode="venice", seed=12)
    solver = CLinearSolver_Schur_HIP(schur_incremental=1)
    x0 = lam.rhs.copy()
    assert solver.Solve_PosDef_Blocky(lam, x0)
    solver.Marginals_Pattern(lam)
    x1 = lam.rhs.copy()
    assert solver.Solve_PosDef_Blocky(lam, x1)
    assert rel_inf(x1, x0) < 1e-13
    # an incremental solve after a covariance call equals a full one
    off, col = lam.block_value_offsets(), block_cols(lam)
    nc, dp = lam.n_matrix_cut, int(lam.cumsum[-1] - lam.cumsum[-2])
    changed = [3, 17, 40]
    vals = lam.values.copy()
    for p in changed:
        i = np.flatnonzero((col == nc + p) & (lam.brow_idx == nc + p))[0]
        vals[off[i]:off[i + 1]] += (0.5 * np.eye(dp)).ravel()
    lam2 = synth.BlockSystem(lam.cumsum, lam.bcol_ptr, lam.brow_idx, vals, lam.rhs, nc)
    solver.Marginal_Columns(lam, [nc + 1, 2])
    solver.Set_Changed_Landmarks(changed)
    x2 = lam2.rhs.copy()
    assert solver.Solve_PosDef_Blocky(lam2, x2)
    x3 = lam2.rhs.copy()
    assert CLinearSolver_Schur_HIP().Solve_PosDef(lam2, x3)
    assert rel_inf(x2, x3) < 1e-10


def test_refusals():
    ba = synth.ba(8, 200, seed=1)
    from slam_plus_plus_amd.hip_solver import _ptr
    h = CLinearSolver_HIP()                                        # a sparse-mode handle
    h.SymbolicDecomposition_Blocky(ba)
    vals = np.ascontiguousarray(ba.values)
    with pytest.raises(NotImplementedError):
        h._check(h._lib.slampp_hip_schur_marginals_pattern(h._h, _ptr(vals), _ptr(np.empty_like(vals))))
    with pytest.raises(NotImplementedError):
        cols = np.array([0], dtype=np.int64)
        h._check(h._lib.slampp_hip_schur_marginal_columns(h._h, _ptr(vals), 1, _ptr(cols), _ptr(np.empty(ba.n_scalars * 8))))
    group = CLinearSolver_Schur_HIP(devices=[0, 0])
    with pytest.raises(NotImplementedError):
        group.Marginals_Pattern(ba)
    with pytest.raises(NotImplementedError):
        group.Marginal_Columns(ba, [0])
    solver = CLinearSolver_Schur_HIP()
    with pytest.raises(ValueError):                                # nothing to reuse yet
        solver.Marginal_Columns(ba, [0], reuse_factor=True)
    n = ba.n_bcols
    for bad in ([n], [-1], [3, 3], []):
        with pytest.raises(ValueError):
            solver.Marginal_Columns(ba, bad)


def test_fallback_answers_as_the_sparse_path():
    rng = np.random.default_rng(4)
    lam = synth.ba(12, 80, k=3, mode="uniform", seed=9)
    M = lam.to_scipy().toarray()
    nc, n_x = lam.n_matrix_cut, int(lam.cumsum[lam.n_matrix_cut])
    for p, q in ((3, 7), (10, 11)):
        a, b = n_x + 3 * p, n_x + 3 * q
        B = 0.05 * rng.standard_normal((3, 3))
        M[a:a + 3, b:b + 3] += B
        M[b:b + 3, a:a + 3] += B.T
    lam2 = system_from_dense(M, np.diff(lam.cumsum), lam.rhs, nc)
    schur, sparse = CLinearSolver_Schur_HIP(), CLinearSolver_HIP()
    cov = schur.Marginals_Pattern(lam2)
    assert np.array_equal(cov, sparse.Marginals_Pattern(lam2))
    cols = [nc + 3, 1, nc + 7]
    X = schur.Marginal_Columns(lam2, cols)
    assert np.array_equal(X, sparse.Marginal_Columns(lam2, cols))
    assert rel_inf(cov, pattern_from_dense(lam2, np.linalg.inv(M))) < TOL
    assert np.array_equal(schur.Marginal_Columns(lam2, cols, reuse_factor=True), X)


def test_repeatable_bitwise():
    lam = synth.ba(40, 500, mode="venice", seed=21)
    nc = lam.n_matrix_cut
    for opts in ({}, {"schur_sparse": 1, "dense_top_nb": 0}):
        solver = CLinearSolver_Schur_HIP(**opts)
        a, b = solver.Marginals_Pattern(lam), solver.Marginals_Pattern(lam)
        assert np.array_equal(a, b)
        cols = [0, nc + 5, 9]
        assert np.array_equal(solver.Marginal_Columns(lam, cols), solver.Marginal_Columns(lam, cols))


def test_full_size_band():
    """C4 band (1000 cameras x 500 000 landmarks): the pattern and six columns from the factor in place -- two code paths --
    agree, and Lambda X = E."""
    lam = synth.ba(1000, 500_000, mode="band")
    solver = CLinearSolver_Schur_HIP()
    cov = solver.Marginals_Pattern(lam)
    nc = lam.n_matrix_cut
    cols = [0, 499, 999, nc + 0, nc + 250_000, nc + 499_999]
    X = solver.Marginal_Columns(lam, cols, reuse_factor=True)
    cs, off, col = lam.cumsum, lam.block_value_offsets(), block_cols(lam)
    j0 = 0
    for c in cols:
        d = int(cs[c + 1] - cs[c])
        Xc = X[:, j0:j0 + d]
        for i in np.flatnonzero(col == c):                         # the stored blocks (r, c) of column c
            r = lam.brow_idx[i]
            blk = cov[off[i]:off[i + 1]].reshape(d, -1)             # column-major d_r x d_c -> rows are the columns
            assert np.abs(Xc[cs[r]:cs[r + 1], :] - blk.T).max() <= 1e-9 * np.abs(blk).max()
        j0 += d
    E = np.zeros_like(X)
    j0 = 0
    for c in cols:
        d = int(cs[c + 1] - cs[c])
        E[cs[c]:cs[c + 1], j0:j0 + d] = np.eye(d)
        j0 += d
    R = lam.to_scipy() @ X - E
    assert np.abs(R).max() < 1e-8
