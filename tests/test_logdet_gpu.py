"""log det Lambda from the Cholesky factor on the device (slampp_hip_logdet / slampp_hip_logdet_device_async), in both modes.

Reference and tolerance.  The test builds the dense M(v) from the packed values on the CPU (the scatter of
torch_solve.dense_from_packed) and computes l_lu = slogdet(M), l_c = 2 sum log diag chol(M) and l_r, the same on the reversed
ordering M[::-1, ::-1].  With spread = the largest difference among the three and sumabs = 2 sum |log diag chol(M)|, the
device value must satisfy |l_gpu - l_c| <= 4 spread + 64 eps sumabs, eps = 2^-52: another elimination order is one more
sample of what the three CPU computations already differ by, and the second term is a floor for summing n logs in another
fixed order.  Where the same factor is summed in two orders (the factor handed back by factorize(), a reused factor, a
damping taken back out) the floor alone is the bound.

The cond_chain6_* fixtures store diagonal blocks that are not exactly symmetric (up to 1.8e-12).  The factor kernels read
the UPPER triangle of a diagonal block (lambda_element() in csrc/sparse_device.inl, as the reference's solvers do), so for
them the reference is built from the upper triangle mirrored; the tolerance stays the same.

Every case prints its measured error, spread and sumabs."""
import ctypes
import dataclasses
import functools
import os

import numpy as np
import pytest

from slam_plus_plus_amd import synth
from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP, CLinearSolver_Schur_HIP, NOT_POSDEF
from golden_util import GOLDEN_DIR
from variant_util import PLAN_OPTIONS, MIXED_SEED

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
TOL = 1e-10                       # the project's bound on a solution's relative error
SPARSE_GOLDENS = ["chain3_n90", "chain6_n60", "chain7_n40", "manhattan_n150", "sphere_8x8", "assembly_se2_n40",
                  "assembly_se3_n40", "dump_chain6_n12", "cond_chain6_1e6", "cond_chain6_1e9", "cond_chain6_1e12"]
SCHUR_GOLDENS = ["ba_12x150_venice", "ba_10x120_band", "dump_ba_5x40", "cond_ba_1e6", "cond_ba_1e9", "cond_ba_1e12",
                 "cond_ba_lm_200cams"]
INDEFINITE = ["indefinite_n40", "cond_chain6_1e9_indefinite", "cond_ba_1e9_indefinite"]
UPPER_TRIANGLE_MIRRORED = ("cond_chain6_1e6", "cond_chain6_1e9", "cond_chain6_1e12")   # (module docstring)
SPARSE_VARIANTS = {"default": {}, "many_stages": PLAN_OPTIONS, "natural_order": {"natural_order": 1}}
FORCED_DENSE_TOP = {"dense_top_nb": 2, "dense_top_min_dim": 0}


@functools.lru_cache(maxsize=None)
def load(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    return synth.BlockSystem(z["cumsum"].astype(np.int64), z["bcol_ptr"].astype(np.int64), z["brow_idx"].astype(np.int32),
                             z["values"], z["rhs"], int(z["n_matrix_cut"]) if "n_matrix_cut" in z.files else 0, name)


def dense_matrix(lam, values=None, upper_mirrored=False):
    """M(v) of the packed values: a stored block (r, c), r < c, at (r, c) and transposed at (c, r), diagonal blocks as stored --
    or, ``upper_mirrored``, from their upper triangle."""
    from slam_plus_plus_amd.torch_solve import _element_rows_cols
    v = lam.values if values is None else values
    row, col, offdiag = _element_rows_cols(lam)
    n = int(lam.cumsum[-1])
    M = np.zeros((n, n))
    M[row, col] = v
    M[col[offdiag], row[offdiag]] = v[offdiag]
    if upper_mirrored:
        M = np.triu(M) + np.triu(M, 1).T
    return M


@dataclasses.dataclass
class Reference:
    l_c: float
    spread: float
    sumabs: float

    @property
    def floor(self):
        return 64 * EPS * self.sumabs

    @property
    def tol(self):
        return 4 * self.spread + self.floor


def reference_of(lam, values=None, upper_mirrored=False):
    M = dense_matrix(lam, values, upper_mirrored)
    sign, l_lu = np.linalg.slogdet(M)
    assert sign == 1.0, lam.name                                   # a positive case
    logs = np.log(np.diag(np.linalg.cholesky(M)))
    l_c = 2 * float(logs.sum())
    l_r = 2 * float(np.log(np.diag(np.linalg.cholesky(M[::-1, ::-1]))).sum())
    three = (float(l_lu), l_c, l_r)
    return Reference(l_c, max(three) - min(three), 2 * float(np.abs(logs).sum()))


@functools.lru_cache(maxsize=None)
def golden_reference(name):
    return reference_of(load(name), upper_mirrored=name in UPPER_TRIANGLE_MIRRORED)


def report(what, value, ref, bound=None):
    err = abs(value - ref.l_c)
    print(f"logdet {what}: error {err:.2e}, spread {ref.spread:.2e}, sumabs {ref.sumabs:.4g}, tolerance {ref.tol:.2e}")
    assert err <= (ref.tol if bound is None else bound), (what, value, ref)


def _dev(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def device_logdet(solver, values_dev, reuse=False):
    """(sync's answer, the double the device call wrote)"""
    import torch
    out = torch.full((1,), 7.0, dtype=torch.float64, device="cuda")
    solver.logdet_device(values_dev.data_ptr() if values_dev is not None else 0, out.data_ptr(), reuse)
    ok = solver.sync()
    return ok, float(out.cpu()[0])


def same_bits(a, b):
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def check_both_entry_points(solver, lam, ref, what):
    """The host call, then the device call twice: the tolerance, and the same bits from the same call."""
    value = solver.Log_Determinant(lam)
    report(what, value, ref)
    vals = _dev(lam.values)
    ok, first = device_logdet(solver, vals)
    ok2, second = device_logdet(solver, vals)
    assert ok and ok2 and same_bits(first, second) and same_bits(first, value), (what, value, first, second)
    return value


# ---- sparse mode ----

@pytest.mark.parametrize("variant", list(SPARSE_VARIANTS))
@pytest.mark.parametrize("name", SPARSE_GOLDENS)
def test_sparse_goldens(name, variant):
    check_both_entry_points(CLinearSolver_HIP(**SPARSE_VARIANTS[variant]), load(name), golden_reference(name), f"{name} [{variant}]")


@pytest.mark.parametrize("tiles", [0, 1])
@pytest.mark.parametrize("nb", [2, 6])
@pytest.mark.parametrize("name", ["sphere_8x8", "manhattan_n150"])
def test_forced_dense_top(name, nb, tiles):
    """Pivots out of the dense matrix of the top separators; its alignment gaps and padding carry identity and are not counted.
    dense_top_nb = 2 puts every column of these systems into the top, 6 leaves the lower part of the tree in the block layout."""
    lam = load(name)
    solver = CLinearSolver_HIP(dense_top_tiles=tiles, **dict(FORCED_DENSE_TOP, dense_top_nb=nb))
    value = check_both_entry_points(solver, lam, golden_reference(name), f"{name} [dense top, nb={nb}, tiles={tiles}]")
    plan = solver.plan()
    n_in_top = int(plan["dim"][plan["dense_pos"] >= 0].sum())
    assert plan["dense_dim"] > 0 and 0 < n_in_top <= plan["dense_dim"]
    assert n_in_top < lam.n_scalars if nb == 6 else n_in_top == lam.n_scalars
    print(f"{name}: {n_in_top} pivots in a dense top of dimension {plan['dense_dim']}")
    # the handle is left as a solve leaves it: another right-hand side with the kept factor
    x = lam.rhs.copy()
    assert solver.Solve_Again(x)
    assert np.abs(dense_matrix(lam) @ x - lam.rhs).max() < 1e-9 * np.abs(lam.rhs).max()
    assert abs(solver.Log_Determinant(lam, reuse_factor=True) - value) <= golden_reference(name).floor


def factor_diagonal_logdet(st, l_values):
    total = []
    for j in range(len(st["dim"])):
        d, off = int(st["dim"][j]), int(st["loff"][st["lptr"][j]])
        total.append(np.log(l_values[off + np.arange(d) * (d + 1)]))
    return 2 * float(np.concatenate(total).sum())


@pytest.mark.parametrize("options", [{}, PLAN_OPTIONS, FORCED_DENSE_TOP], ids=["default", "many_stages", "dense_top"])
@pytest.mark.parametrize("name", ["chain6_n60", "sphere_8x8", "manhattan_n150"])
def test_agrees_with_the_factor_handed_back(name, options):
    """The same L, summed on the host in another order: the floor alone."""
    lam, ref = load(name), golden_reference(name)
    solver = CLinearSolver_HIP(**options)
    ok, st, l_values = solver.factorize(lam)
    assert ok
    host = factor_diagonal_logdet(st, l_values)
    value = solver.Log_Determinant(lam)
    print(f"logdet {name}: device {value!r}, from factorize() {host!r}, difference {abs(value - host):.2e}, floor {ref.floor:.2e}")
    assert abs(value - host) <= ref.floor


def mixed_system():
    from test_sparse_gpu import random_system
    lam, _ = random_system(MIXED_SEED)
    assert len(set(np.diff(lam.cumsum).tolist())) > 1 and int(np.diff(lam.cumsum).max()) <= 8
    return dataclasses.replace(lam, name="mixed")


def wide_system(dims):
    """Block columns of two widths, one of them above 8: the generator of test_sparse_gpu's wide-column test."""
    rng = np.random.default_rng(sum(dims))
    n = 60
    d = np.where(rng.random(n) < 0.4, dims[0], dims[1])
    cs = np.concatenate([[0], np.cumsum(d)]).astype(np.int64)
    a, b = rng.integers(0, n, 90), rng.integers(0, n, 90)
    pairs = set(zip(range(n - 1), range(1, n))) | {(min(x, y), max(x, y)) for x, y in zip(a, b) if x != y}
    M = np.zeros((cs[-1], cs[-1]))
    for r, c in pairs:
        B = 0.3 * rng.standard_normal((d[r], d[c]))
        M[cs[r]:cs[r + 1], cs[c]:cs[c + 1]] = B
        M[cs[c]:cs[c + 1], cs[r]:cs[r + 1]] = B.T
    M += np.eye(cs[-1]) * (np.abs(M).sum(axis=1).max() + 1.0)
    bcol_ptr, brow, vals = [0], [], []
    for c in range(n):
        for r in range(c + 1):
            if r == c or (r, c) in pairs:
                brow.append(r)
                vals.append(M[cs[r]:cs[r + 1], cs[c]:cs[c + 1]].T.ravel())
        bcol_ptr.append(len(brow))
    return synth.BlockSystem(cs, np.asarray(bcol_ptr, dtype=np.int64), np.asarray(brow, dtype=np.int32), np.concatenate(vals),
                             rng.standard_normal(int(cs[-1])), 0, f"wide{dims}")


@functools.lru_cache(maxsize=None)
def synthetic(kind):
    lam = mixed_system() if kind == "mixed" else wide_system(kind)
    return lam, reference_of(lam)


@pytest.mark.parametrize("variant", list(SPARSE_VARIANTS))
@pytest.mark.parametrize("kind", ["mixed", (11, 3), (9, 9)], ids=["mixed_2_to_8", "wide_11_3", "wide_9_9"])
def test_mixed_and_wide_block_columns(kind, variant):
    """Block sizes 2 .. 8 mixed; block columns wider than 8, which are factored in pieces (the table is built over the pieces)."""
    lam, ref = synthetic(kind)
    check_both_entry_points(CLinearSolver_HIP(**SPARSE_VARIANTS[variant]), lam, ref, f"{lam.name} [{variant}]")


@pytest.mark.parametrize("options", [{}, FORCED_DENSE_TOP], ids=["default", "dense_top"])
@pytest.mark.parametrize("name", ["chain6_n60", "manhattan_n150"])
def test_sparse_reuse_and_the_handle_afterwards(name, options):
    lam, ref = load(name), golden_reference(name)
    x_ref = np.linalg.solve(dense_matrix(lam), lam.rhs)
    solver = CLinearSolver_HIP(**options)
    solver.SymbolicDecomposition_Blocky(lam)
    vals = _dev(lam.values)
    with pytest.raises(ValueError, match="no valid factorization"):          # nothing factored yet
        device_logdet(solver, vals, reuse=True)
    ok, fresh = device_logdet(solver, vals)
    assert ok
    report(f"{name} fresh", fresh, ref)
    # solve_again gives the solver's usual answer after a log-determinant that factored
    x = _dev(2.0 * lam.rhs)
    solver.solve_again_device(x.data_ptr())
    assert solver.sync()
    assert np.abs(x.cpu().numpy() - 2.0 * x_ref).max() < TOL * np.abs(2.0 * x_ref).max()
    # the factor a solve of the same values left, read without factoring; the values are not needed
    eta = _dev(lam.rhs)
    assert solver.factor_solve_device(vals.data_ptr(), eta.data_ptr())
    ok, reused = device_logdet(solver, vals, reuse=True)
    ok2, reused_null = device_logdet(solver, None, reuse=True)
    assert ok and ok2 and same_bits(reused, reused_null)
    print(f"logdet {name}: fresh {fresh!r}, reused {reused!r}, difference {abs(fresh - reused):.2e}, floor {ref.floor:.2e}")
    assert abs(reused - fresh) <= ref.floor
    assert abs(solver.Log_Determinant(lam, reuse_factor=True) - fresh) <= ref.floor
    # null pointers
    with pytest.raises(ValueError, match="null"):
        solver.logdet_device(0, eta.data_ptr(), False)
    with pytest.raises(ValueError, match="null"):
        solver.logdet_device(vals.data_ptr(), 0, True)


# ---- not positive definite ----

def _solver_for(lam, **options):
    return CLinearSolver_Schur_HIP(**options) if lam.n_matrix_cut else CLinearSolver_HIP()


@pytest.mark.parametrize("name", INDEFINITE)
def test_not_positive_definite(name):
    lam = load(name)
    with pytest.raises(np.linalg.LinAlgError):                               # a negative case
        np.linalg.cholesky(dense_matrix(lam, upper_mirrored=True))
    solver = _solver_for(lam, schur_keep=1)
    solver.SymbolicDecomposition_Blocky(lam)
    values = np.ascontiguousarray(lam.values)
    out = ctypes.c_double(7.0)
    rc = solver._lib.slampp_hip_logdet(solver._h, values.ctypes.data_as(ctypes.c_void_p), 0, ctypes.byref(out))
    assert rc == NOT_POSDEF and np.isnan(out.value)
    assert np.isnan(solver.Log_Determinant(lam))
    vals = _dev(lam.values)
    ok, value = device_logdet(solver, vals)                                  # NaN decided on the device; sync says why
    assert ok is False and np.isnan(value)
    with pytest.raises(ValueError):                                          # the failed factorization left nothing to reuse
        device_logdet(solver, vals, reuse=True)
    with pytest.raises(ValueError):
        solver.Log_Determinant(lam, reuse_factor=True)
    # the flag is clean again: the handle goes on with a good matrix of the same structure
    good = {"indefinite_n40": None, "cond_chain6_1e9_indefinite": "cond_chain6_1e9", "cond_ba_1e9_indefinite": "cond_ba_1e9"}[name]
    if good is not None and np.array_equal(load(good).brow_idx, lam.brow_idx):
        report(f"{good} after {name}", solver.Log_Determinant(load(good)), golden_reference(good))


# ---- Schur mode ----

SCHUR_REDUCED = {"dense_S": {"schur_sparse": 0}, "sparse_S": {"schur_sparse": 1}}


@pytest.mark.parametrize("reduced", list(SCHUR_REDUCED))
@pytest.mark.parametrize("name", SCHUR_GOLDENS)
def test_schur_goldens(name, reduced):
    """log det Lambda = log det S + sum log det C_p, S factored dense or by the sparse block path."""
    lam = load(name)
    assert lam.n_matrix_cut > 0
    solver = CLinearSolver_Schur_HIP(**SCHUR_REDUCED[reduced])
    check_both_entry_points(solver, lam, golden_reference(name), f"{name} [{reduced}]")
    assert (solver.reduced_stats()["n_bcols"] > 0) == (reduced == "sparse_S")


@functools.lru_cache(maxsize=None)
def synthetic_ba(cam_dim, pt_dim):
    lam = synth.ba(12, 90, k=3, mode="uniform", seed=41, cam_dim=cam_dim, pt_dim=pt_dim)   # test_schur_block_sizes_gpu.system()
    dims = np.diff(lam.cumsum)
    assert lam.n_matrix_cut == 12 and np.all(dims[:12] == cam_dim) and np.all(dims[12:] == pt_dim)
    return lam, reference_of(lam)


@pytest.mark.parametrize("reduced", list(SCHUR_REDUCED))
@pytest.mark.parametrize("cam_dim,pt_dim", [(7, 3), (3, 2)])
def test_schur_other_block_sizes(cam_dim, pt_dim, reduced):
    lam, ref = synthetic_ba(cam_dim, pt_dim)
    check_both_entry_points(CLinearSolver_Schur_HIP(**SCHUR_REDUCED[reduced]), lam, ref, f"ba ({cam_dim}, {pt_dim}) [{reduced}]")


@pytest.mark.parametrize("reduced", list(SCHUR_REDUCED))
def test_schur_reuse_rule(reduced):
    name = "ba_12x150_venice"
    lam, ref = load(name), golden_reference(name)
    x_ref = np.linalg.solve(dense_matrix(lam), lam.rhs)
    vals = _dev(lam.values)
    fresh = CLinearSolver_Schur_HIP(**SCHUR_REDUCED[reduced]).Log_Determinant(lam)
    # with schur_keep, after a solve: the kept factor is read
    solver = CLinearSolver_Schur_HIP(schur_keep=1, **SCHUR_REDUCED[reduced])
    eta = lam.rhs.copy()
    assert solver.Solve_PosDef(lam, eta)
    ok, reused = device_logdet(solver, vals, reuse=True)
    print(f"logdet {name} [{reduced}]: fresh {fresh!r}, reused {reused!r}, difference {abs(fresh - reused):.2e}, floor {ref.floor:.2e}")
    assert ok and abs(reused - fresh) <= ref.floor
    assert abs(solver.Log_Determinant(lam, reuse_factor=True) - fresh) <= ref.floor
    x = 3.0 * lam.rhs                                                        # reading it changed nothing: solve_again still works
    assert solver.Solve_Again(x) and np.abs(x - 3.0 * x_ref).max() < TOL * np.abs(3.0 * x_ref).max()
    # the values are required in Schur mode, reused factor or not
    with pytest.raises(ValueError, match="null values"):
        device_logdet(solver, None, reuse=True)
    with pytest.raises(ValueError, match="null values"):
        device_logdet(solver, None, reuse=False)
    # a log-determinant that factors leaves what a solve leaves: solve_again and another reuse are valid after it
    ok, again = device_logdet(solver, vals)
    assert ok and abs(again - fresh) <= ref.floor
    x = -lam.rhs
    assert solver.Solve_Again(x) and np.abs(x + x_ref).max() < TOL * np.abs(x_ref).max()
    ok, reused = device_logdet(solver, vals, reuse=True)
    assert ok and abs(reused - fresh) <= ref.floor
    # what a Schur covariance call left is not a factor to read: its dense route holds inv(L)
    solver.Marginals_Pattern(lam)
    with pytest.raises(ValueError, match=r"inv\(L\)"):
        device_logdet(solver, vals, reuse=True)
    # without schur_keep a solve keeps nothing
    plain = CLinearSolver_Schur_HIP(**SCHUR_REDUCED[reduced])
    assert plain.Solve_PosDef(lam, lam.rhs.copy())
    with pytest.raises(ValueError, match="schur_keep"):
        device_logdet(plain, vals, reuse=True)
    with pytest.raises(ValueError, match="schur_keep"):
        plain.Log_Determinant(lam, reuse_factor=True)
    report(f"{name} [{reduced}] after the refusals", plain.Log_Determinant(lam), ref)


def test_a_handle_over_several_devices_is_refused():
    lam = load("ba_10x120_band")
    solver = CLinearSolver_Schur_HIP(devices=[0, 0], schur_keep=1)
    assert solver.Solve_PosDef(lam, lam.rhs.copy())
    with pytest.raises(NotImplementedError):
        solver.logdet_device(_dev(lam.values).data_ptr(), _dev(np.zeros(1)).data_ptr(), False)
    with pytest.raises(NotImplementedError):
        solver.Log_Determinant(lam)


def test_schur_handle_without_a_landmark_part_answers_as_the_sparse_path():
    name = "chain6_n60"
    lam, ref = load(name), golden_reference(name)
    solver = CLinearSolver_Schur_HIP()
    value = check_both_entry_points(solver, lam, ref, f"{name} [schur_fallback]")
    assert same_bits(value, CLinearSolver_HIP().Log_Determinant(lam))
    assert abs(solver.Log_Determinant(lam, reuse_factor=True) - value) <= ref.floor     # the sparse path's reuse rule


# ---- damping ----

@pytest.mark.parametrize("name", ["chain6_n60", "ba_10x120_band"])
def test_damping_increases_the_log_determinant(name):
    lam, ref = load(name), golden_reference(name)
    solver = _solver_for(lam)
    solver.SymbolicDecomposition_Blocky(lam)
    vals = _dev(lam.values)
    ok, before = device_logdet(solver, vals)
    alpha = 0.5
    solver.apply_damping_device_async(vals.data_ptr(), alpha, 0, lam.n_bcols)
    ok2, damped = device_logdet(solver, vals)
    solver.apply_damping_device_async(vals.data_ptr(), -alpha, 0, lam.n_bcols)
    ok3, after = device_logdet(solver, vals)
    print(f"logdet {name}: {before!r} -> +{alpha}: {damped!r} -> back: {after!r} (difference {abs(after - before):.2e}, floor {ref.floor:.2e})")
    assert ok and ok2 and ok3 and damped > before
    damped_ref = reference_of(lam, values=vals_plus_alpha(lam, alpha))
    report(f"{name} + {alpha} I", damped, damped_ref)
    assert abs(after - before) <= ref.floor


def vals_plus_alpha(lam, alpha):
    from variant_util import damped
    return damped(lam, alpha).values
