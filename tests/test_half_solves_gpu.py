"""The two substitutions of a k-column solve one at a time (slampp_hip_solve_half_columns / _device_async) and the fixed-order
tall-skinny product (slampp_hip_gram_device_async).

Reference, independent of the device factor: numpy's Cholesky factor of the dense Lambda permuted by
factor_structure()["perm"] (as test_sparse_gpu.test_factorize_returns_the_cholesky_factor builds it), then
scipy.linalg.solve_triangular.  y = L^-1 P b, x = P^T L^-T y and G = Y^T Y are held to the project's 1e-10, relative to the
reference's largest entry in that column (in G).  k runs over 1, 10, 11, 48, 49: on either side of the ten right-hand sides a
wave carries at 6 x 6 blocks and of the 48 columns of a pass; packed, and with five doubles of padding behind every column,
which must come back untouched.

Bits: a forward call followed by a backward call on its result against slampp_hip_solve_columns_device_async, in every
variant (the dense top included); the same call twice; column c of an 11-column call against the same vector alone (no dense
top); a column of NaN beside ten clean ones.  Then the refusals with their texts, and the host form.

One handle and one factorization per test; the references of a system are computed once.  Every test prints its worst figures."""
import functools

import numpy as np
import pytest

from slam_plus_plus_amd.hip_solver import (CLinearSolver_HIP, CLinearSolver_Schur_HIP, SOLVE_MAX_COLUMNS, HALF_FORWARD,
                                           HALF_BACKWARD, GRAM_MAX_COLUMNS, GRAM_CHUNK_ROWS)
from golden_util import load_golden
from variant_util import PLAN_OPTIONS, MIXED_SEED

pytestmark = pytest.mark.gpu

TOL = 1e-10                        # the project's bound
KS = (1, 10, 11, 48, 49)
K_MAX = max(KS)
PAD = 5
SENTINEL = -777.25
SYSTEMS = ["chain3_n90", "chain6_n60", "chain7_n40", "manhattan_n150", "sphere_8x8", "mixed"]
OPTIONS = {"default": {}, "many_stages": PLAN_OPTIONS, "natural_order": {"natural_order": 1},
           "dense_top": {"dense_top_nb": 2, "dense_top_min_dim": 0}}


@functools.lru_cache(maxsize=None)
def system(name):
    """(the system, its dense Lambda, K_MAX seeded right-hand sides with eta in row 0)"""
    if name == "mixed":
        from test_sparse_gpu import random_system
        lam, _ = random_system(MIXED_SEED)
        dims = np.diff(lam.cumsum)
        assert len(set(dims.tolist())) > 1 and int(dims.max()) <= 8
    else:
        lam, _ = load_golden(name)
    A = lam.to_scipy().toarray()
    B = np.random.default_rng(4242 + len(name)).standard_normal((K_MAX, lam.n_scalars))
    B[0] = lam.rhs
    A.setflags(write=False)
    B.setflags(write=False)
    return lam, A, B


@functools.lru_cache(maxsize=8)
def _reference(name, perm_bytes):
    """(idx, Y, X, G) for all K_MAX rows of the system's B: idx[s] = the caller's scalar at the factor's scalar s."""
    from scipy.linalg import solve_triangular
    lam, A, B = system(name)
    perm = np.frombuffer(perm_bytes, dtype=np.int32)
    cs = lam.cumsum
    idx = np.concatenate([np.arange(cs[o], cs[o + 1]) for o in perm])
    L = np.linalg.cholesky(A[np.ix_(idx, idx)])
    Y = solve_triangular(L, B[:, idx].T, lower=True)                      # (n, K): columns y
    Xp = solve_triangular(L, Y, lower=True, trans="T")
    X = np.empty_like(Xp)
    X[idx] = Xp
    return idx, np.ascontiguousarray(Y.T), np.ascontiguousarray(X.T), Y.T @ Y


def reference(name, solver):
    return _reference(name, solver.factor_structure()["perm"].astype(np.int32).tobytes())


def _dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def column_err(got, ref):
    """max over the rows (the call's columns) of max |got - ref| / max |ref|"""
    return float((np.abs(got - ref).max(axis=1) / np.abs(ref).max(axis=1)).max())


def device_call(solver, rows, ld, call):
    """``call(ptr, ld, k)`` on a copy of the rows at the leading dimension ld: (result, what stands in the padding)."""
    import torch
    k, n = rows.shape
    buf = torch.full((k, ld), SENTINEL, dtype=torch.float64, device="cuda")
    buf[:, :n] = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    torch.cuda.synchronize()                                             # (torch fills on its own stream, the library reads on the handle's)
    generation = solver.factor_generation
    call(buf.data_ptr(), ld, k)
    assert solver.sync() and solver.factor_generation == generation      # (it installs no factor)
    out = buf.cpu().numpy()
    return out[:, :n].copy(), out[:, n:].copy()


def half(solver, rows, ld, which):
    return device_call(solver, rows, ld, lambda p, l, k: solver.solve_half_columns_device(p, l, k, which))


def whole(solver, rows, ld):
    return device_call(solver, rows, ld, solver.solve_columns_device)


def gram(solver, A, B=None, lda=None, ldb=None, ldo=None):
    """out = A^T B for row-major (k, n) arrays (their rows are the operands' columns); B = None: the same device array twice."""
    import torch
    ka, n = A.shape
    lda = lda or max(n, 1)
    a = torch.full((ka, lda), SENTINEL, dtype=torch.float64, device="cuda")
    a[:, :n] = torch.from_numpy(np.ascontiguousarray(A)).cuda()
    if B is None:
        b, kb, ldb = a, ka, lda
    else:
        kb, ldb = B.shape[0], ldb or max(n, 1)
        b = torch.full((kb, ldb), SENTINEL, dtype=torch.float64, device="cuda")
        b[:, :n] = torch.from_numpy(np.ascontiguousarray(B)).cuda()
    ldo = ldo or ka
    out = torch.full((kb, ldo), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    solver.gram_device(a.data_ptr(), lda, ka, b.data_ptr(), ldb, kb, n, out.data_ptr(), ldo)
    assert solver.sync()
    got = out.cpu().numpy()
    assert np.all(got[:, ka:] == SENTINEL)
    return got[:, :ka].T.copy()                                           # (i, j)


def factored_solver(lam, options):
    solver = CLinearSolver_HIP(**options)
    solver.SymbolicDecomposition_Blocky(lam)
    vals, eta = _dev(lam.values), _dev(lam.rhs)
    assert solver.factor_solve_device(vals.data_ptr(), eta.data_ptr())
    return solver


# ---- the halves ----

@pytest.mark.parametrize("variant", list(OPTIONS))
@pytest.mark.parametrize("name", SYSTEMS)
def test_halves(name, variant):
    import torch
    lam, _, B = system(name)
    n = lam.n_scalars
    solver = factored_solver(lam, OPTIONS[variant])
    assert (solver.plan()["dense_dim"] > 0) == (variant == "dense_top")
    idx, Y_ref, X_ref, G_ref = reference(name, solver)
    worst = {"y": 0.0, "x": 0.0, "G": 0.0, "diag": 0.0}
    for k in KS:
        for ld in (n, n + PAD):
            Y, pad = half(solver, B[:k], ld, HALF_FORWARD)
            assert np.all(pad == SENTINEL), (k, ld)
            X, pad = half(solver, Y, ld, HALF_BACKWARD)
            assert np.all(pad == SENTINEL), (k, ld)
            figures = {"y": column_err(Y, Y_ref[:k]), "x": column_err(X, X_ref[:k])}
            X_whole, _ = whole(solver, B[:k], ld)
            assert same_bits(X, X_whole), (k, ld)                       # the two halves are the whole, bit for bit
            again, _ = half(solver, B[:k], ld, HALF_FORWARD)
            assert same_bits(Y, again), (k, ld)                         # the same call twice
            again, _ = half(solver, Y, ld, HALF_BACKWARD)
            assert same_bits(X, again), (k, ld)
            if k <= GRAM_MAX_COLUMNS and ld == n:
                G = gram(solver, Y)
                figures["G"] = float(np.abs(G - G_ref[:k, :k]).max() / np.abs(G_ref[:k, :k]).max())
                assert same_bits(G, G.T)
                # the diagonal against the fixed-order dot product: both sum n products of about |y|^2 / n each in fp64
                Yd = _dev(Y)
                dots = torch.zeros(k, dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()
                for c in range(k):
                    solver.dot_device(Yd.data_ptr() + 8 * c * n, Yd.data_ptr() + 8 * c * n, n, dots.data_ptr() + 8 * c)
                assert solver.sync()
                d = dots.cpu().numpy()
                figures["diag"] = float((np.abs(np.diag(G) - d) / d).max())
                assert figures["diag"] < n * np.finfo(np.float64).eps   # (two summation orders of n positive terms)
            for what, f in figures.items():
                worst[what] = max(worst[what], f)
            assert all(figures[w] < TOL for w in ("y", "x", "G") if w in figures), (k, ld, figures)
    print(f"half solves {name} [{variant}]: worst y {worst['y']:.2e}, x {worst['x']:.2e}, G {worst['G']:.2e}, "
          f"diag(G) against dot {worst['diag']:.2e}")
    # a column of NaN reaches no other column, in either half
    for which, rows in ((HALF_FORWARD, B[:11]), (HALF_BACKWARD, Y_ref[:11])):
        clean, _ = half(solver, rows, n, which)
        dirty_rows = rows.copy()
        dirty_rows[4] = np.nan
        dirty, _ = half(solver, dirty_rows, n, which)
        others = [c for c in range(11) if c != 4]
        assert np.all(np.isnan(dirty[4])) and np.all(np.isfinite(dirty[others]))
        assert same_bits(dirty[others], clean[others])
        after, _ = half(solver, rows, n, which)                          # and nothing of it stays behind
        assert same_bits(after, clean)
        if variant != "dense_top":                                       # (no dense top) a column does not depend on its company
            for c in range(11):
                alone, _ = half(solver, rows[c:c + 1], n, which)
                assert same_bits(alone[0], clean[c]), (which, c)


# ---- the product ----

GRAM_ROWS = (1, 63, 64, 65, GRAM_CHUNK_ROWS - 1, GRAM_CHUNK_ROWS, GRAM_CHUNK_ROWS + 1, 3 * GRAM_CHUNK_ROWS + 1)


def gram_bound(A, B, n):
    """n eps times the largest sum of absolute products: the classical bound of a length-n dot product in any order."""
    return n * np.finfo(np.float64).eps * float((np.abs(A) @ np.abs(B).T).max()) + np.finfo(np.float64).tiny


def test_gram_against_numpy():
    solver = CLinearSolver_HIP()                                         # (any handle: no structure, no factor)
    rng = np.random.default_rng(77)
    worst = 0.0
    for n in GRAM_ROWS:
        for k in (1, 7, 48):
            A = rng.standard_normal((k, n))
            G = gram(solver, A)
            ref = A @ A.T
            err = float(np.abs(G - ref).max())
            worst = max(worst, err / gram_bound(A, A, n))
            assert err < gram_bound(A, A, n) and err < TOL * np.abs(ref).max(), (n, k, err)
            assert same_bits(G, G.T), (n, k)                             # a == b: bitwise symmetric
            assert same_bits(G, gram(solver, A)), (n, k)                 # two calls: the same bits
    print(f"gram: worst error {worst:.2e} of the n eps sum |a||b| bound")
    # a != b, different column counts and leading dimensions, a padded output
    n = GRAM_CHUNK_ROWS + 65
    A, B = rng.standard_normal((7, n)), rng.standard_normal((48, n))
    G = gram(solver, A, B, lda=n + 3, ldb=n + 11, ldo=9)
    assert G.shape == (7, 48) and np.abs(G - A @ B.T).max() < gram_bound(A, B, n)
    assert same_bits(G, gram(solver, A, B, lda=n, ldb=n + 1, ldo=7))     # the layout does not change the sums
    assert same_bits(G.T, gram(solver, B, A))                            # out(i, j) of (a, b) is out(j, i) of (b, a)


def test_gram_refusals():
    import torch
    solver = CLinearSolver_HIP()
    a = torch.zeros((GRAM_MAX_COLUMNS + 1, 100), dtype=torch.float64, device="cuda")
    out = torch.zeros((GRAM_MAX_COLUMNS + 1) ** 2, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    p, o = a.data_ptr(), out.data_ptr()
    for ka, kb in ((GRAM_MAX_COLUMNS + 1, 1), (1, GRAM_MAX_COLUMNS + 1), (0, 1), (1, 0)):
        with pytest.raises(ValueError, match="SLAMPP_HIP_GRAM_MAX_COLUMNS"):
            solver.gram_device(p, 100, ka, p, 100, kb, 100, o, max(ka, 1))
    with pytest.raises(ValueError, match="leading dimension below n_ka"):
        solver.gram_device(p, 100, 3, p, 100, 3, 100, o, 2)
    with pytest.raises(ValueError, match="leading dimension below n_rows"):
        solver.gram_device(p, 99, 3, p, 100, 3, 100, o, 3)
    with pytest.raises(ValueError, match="null"):
        solver.gram_device(0, 100, 3, p, 100, 3, 100, o, 3)
    with pytest.raises(ValueError, match="null"):
        solver.gram_device(p, 100, 3, p, 100, 3, 100, 0, 3)
    with pytest.raises(ValueError, match="overlaps"):
        solver.gram_device(p, 100, 3, p, 100, 3, 100, p + 8, 3)
    solver.gram_device(p, 0, 1, p, 0, 1, 100, o, 1)                      # one column: the leading dimensions are not read
    solver.gram_device(p, 100, 3, p, 100, 3, 0, o, 3)                    # no rows: zeros
    assert solver.sync() and float(out.abs().max()) == 0.0


# ---- refusals ----

def test_refusals():
    lam, _, B = system("chain6_n60")
    n = lam.n_scalars
    buf = _dev(B[:3])
    solver = CLinearSolver_HIP()
    solver.SymbolicDecomposition_Blocky(lam)
    for which in (HALF_FORWARD, HALF_BACKWARD):
        with pytest.raises(ValueError, match="solve_half_columns: no valid factorization"):   # nothing factored yet
            solver.solve_half_columns_device(buf.data_ptr(), n, 3, which)
        with pytest.raises(ValueError, match="solve_half_columns: no valid factorization"):
            solver.Solve_Half_Columns(B[:3].copy(), which)
    vals, eta = _dev(lam.values), _dev(lam.rhs)
    assert solver.factor_solve_device(vals.data_ptr(), eta.data_ptr())
    for which in (2, -1):
        with pytest.raises(ValueError, match="SLAMPP_HIP_HALF_FORWARD or SLAMPP_HIP_HALF_BACKWARD"):
            solver.solve_half_columns_device(buf.data_ptr(), n, 3, which)
    for which in (HALF_FORWARD, HALF_BACKWARD):
        for k in (0, SOLVE_MAX_COLUMNS + 1):
            with pytest.raises(ValueError, match="SLAMPP_HIP_SOLVE_MAX_COLUMNS"):
                solver.solve_half_columns_device(buf.data_ptr(), n, k, which)
        with pytest.raises(ValueError, match="leading dimension"):
            solver.solve_half_columns_device(buf.data_ptr(), n - 1, 2, which)
        with pytest.raises(ValueError, match="null"):
            solver.solve_half_columns_device(0, n, 3, which)
        solver.solve_half_columns_device(buf.data_ptr(), 0, 1, which)    # one column: the leading dimension is not read
    assert solver.sync()
    # a factorization that fails leaves nothing to solve from
    bad, _ = load_golden("indefinite_n40")
    failing = CLinearSolver_HIP()
    assert failing.Solve_PosDef(bad, bad.rhs.copy()) is False
    with pytest.raises(ValueError, match="solve_half_columns: no valid factorization"):
        failing.solve_half_columns_device(_dev(np.zeros((2, bad.n_scalars))).data_ptr(), bad.n_scalars, 2, HALF_FORWARD)


def test_schur_mode_is_refused_and_says_why():
    lam, _ = load_golden("ba_10x120_band")
    rows = np.ones((2, lam.n_scalars))
    buf = _dev(rows)
    solver = CLinearSolver_Schur_HIP(schur_keep=1)
    assert solver.Solve_PosDef(lam, lam.rhs.copy())
    generation = solver.factor_generation
    for which in (HALF_FORWARD, HALF_BACKWARD):
        with pytest.raises(NotImplementedError, match="solve_half_columns: not in Schur mode.*block factor"):
            solver.solve_half_columns_device(buf.data_ptr(), lam.n_scalars, 2, which)
        with pytest.raises(NotImplementedError, match="Schur mode"):
            solver.Solve_Half_Columns(rows.copy(), which)
    assert solver.sync() and solver.factor_generation == generation and same_bits(buf.cpu().numpy(), rows)
    plain = CLinearSolver_Schur_HIP()                                    # no kept factor: the validity rule of solve_again first
    assert plain.Solve_PosDef(lam, lam.rhs.copy())
    with pytest.raises(ValueError, match="solve_half_columns.*schur_keep"):
        plain.solve_half_columns_device(buf.data_ptr(), lam.n_scalars, 2, HALF_FORWARD)


def test_schur_handle_that_took_the_sparse_path_is_accepted():
    """A Schur handle whose analysis fell back to the sparse path (a system without a landmark part) answers as the sparse
    path does: both halves against the reference, and their bits against solve_columns_device."""
    lam, _, B = system("chain6_n60")
    n = lam.n_scalars
    solver = CLinearSolver_Schur_HIP()
    assert solver.Solve_PosDef(lam, lam.rhs.copy())
    idx, Y_ref, X_ref, _ = reference("chain6_n60", solver)
    Y, _ = half(solver, B[:11], n, HALF_FORWARD)
    X, _ = half(solver, Y, n, HALF_BACKWARD)
    errs = (column_err(Y, Y_ref[:11]), column_err(X, X_ref[:11]))
    print(f"half solves chain6_n60 [Schur handle on the sparse path]: y {errs[0]:.2e}, x {errs[1]:.2e}")
    assert max(errs) < TOL
    X_whole, _ = whole(solver, B[:11], n)
    assert same_bits(X, X_whole)


def test_block_columns_wider_than_8_are_refused():
    from test_logdet_gpu import wide_system
    lam = wide_system((12, 3))
    assert int(np.diff(lam.cumsum).max()) == 12
    solver = factored_solver(lam, {"natural_order": 1})
    buf = _dev(np.ones((2, lam.n_scalars)))
    for which in (HALF_FORWARD, HALF_BACKWARD):
        with pytest.raises(NotImplementedError, match="solve_half_columns: block columns wider than 8"):
            solver.solve_half_columns_device(buf.data_ptr(), lam.n_scalars, 2, which)


# ---- the host form ----

def test_host_form():
    lam, _, B = system("chain6_n60")
    n = lam.n_scalars
    solver = factored_solver(lam, {})
    idx, Y_ref, X_ref, _ = reference("chain6_n60", solver)
    k = K_MAX                                                            # (49 columns: two groups through device memory)
    Y_dev, _ = half(solver, B[:k], n, HALF_FORWARD)
    Y = B[:k].copy()
    assert solver.Solve_Half_Columns(Y, HALF_FORWARD)
    assert same_bits(Y, Y_dev) and column_err(Y, Y_ref[:k]) < TOL
    X_dev, _ = half(solver, Y_dev, n, HALF_BACKWARD)
    X = Y.copy()
    assert solver.Solve_Half_Columns(X, HALF_BACKWARD)
    assert same_bits(X, X_dev) and column_err(X, X_ref[:k]) < TOL
    with pytest.raises(ValueError):
        solver.Solve_Half_Columns(B[:2, :-1].copy(), HALF_FORWARD)
    with pytest.raises(ValueError):
        solver.Solve_Half_Columns(np.zeros((SOLVE_MAX_COLUMNS + 1, n)), HALF_FORWARD)
