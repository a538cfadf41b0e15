"""y = alpha Lambda x + beta y on the device (slampp_hip_multiply / _multiply_device_async) and the fixed-order dot product
(slampp_hip_dot_device_async): against scipy on every golden system, both row regimes (short rows; long rows cut into
chunks), mixed block dimensions, a block column wider than the unrolled kernels take, and bit-reproducibility."""
import numpy as np
import pytest

from slam_plus_plus_amd import synth, hip_solver
from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP, MULTIPLY_CHUNK, MULTIPLY_LONG_ROW
from golden_util import golden_names, dump_names, load_golden, load_dump, rel_inf

pytestmark = pytest.mark.gpu

TOL = 1e-13          # every y entry is a sum of at most a few hundred products of O(1) numbers
SYSTEMS = golden_names() + dump_names()


def _load(name):
    return load_dump(name)[0] if name.startswith("dump_") else load_golden(name)[0]


def _randomize(lam, seed):
    """Random values on a structure, the diagonal blocks symmetric (both triangles stored, as the solver reads them)."""
    rng = np.random.default_rng(seed)
    lam.values = rng.standard_normal(lam.values.shape[0])
    off, dims = lam.block_value_offsets(), np.diff(lam.cumsum)
    cols = np.repeat(np.arange(lam.n_bcols), np.diff(lam.bcol_ptr))
    for k in np.nonzero(lam.brow_idx == cols)[0]:
        d = int(dims[cols[k]])
        B = lam.values[off[k]:off[k + 1]].reshape(d, d)
        lam.values[off[k]:off[k + 1]] = (B + B.T).ravel()
    lam.rhs = rng.standard_normal(lam.n_scalars)
    return lam


def _device_product(solver, lam, x, alpha=1.0, beta=0.0, y0=None):
    """The device entry point on torch memory; the structure must be on the handle already."""
    import torch
    vals = torch.tensor(lam.values, device="cuda")
    xd = torch.tensor(x, device="cuda")
    yd = torch.full((lam.n_scalars,), float("nan"), dtype=torch.float64, device="cuda") if y0 is None else torch.tensor(y0, device="cuda")
    solver.multiply_device(vals.data_ptr(), xd.data_ptr(), yd.data_ptr(), alpha, beta)
    assert solver.sync()
    return yd


@pytest.mark.parametrize("name", SYSTEMS)
def test_product_matches_scipy_on_the_golden_systems(name):
    lam = _load(name)
    x = np.random.default_rng(5).standard_normal(lam.n_scalars)
    ref = lam.to_scipy() @ x
    solver = CLinearSolver_HIP()
    y = solver.Multiply(lam, x)
    err = rel_inf(y, ref)
    print(f"{name}: Multiply vs scipy rel-inf {err:.2e}")
    assert err < TOL
    yd = _device_product(solver, lam, x)                     # the device entry point: the same bits, twice
    assert np.array_equal(yd.cpu().numpy(), y)
    import torch
    assert torch.equal(yd, _device_product(solver, lam, x))


@pytest.mark.parametrize("name", ["chain6_n60", "ba_12x150_venice"])
def test_alpha_beta_and_the_residual(name):
    lam = _load(name)
    x = np.random.default_rng(6).standard_normal(lam.n_scalars)
    A = lam.to_scipy()
    solver = CLinearSolver_HIP()
    y = np.full(lam.n_scalars, np.nan)
    assert solver.Multiply(lam, x, y, alpha=2.5, beta=0.0) is y          # beta = 0 does not read y
    assert rel_inf(y, 2.5 * (A @ x)) < TOL
    r = lam.rhs.copy()
    solver.Multiply(lam, x, r, alpha=-1.0, beta=1.0)                     # the residual eta - Lambda x
    ref = lam.rhs - A @ x
    assert np.abs(r - ref).max() < TOL * max(np.abs(A @ x).max(), np.abs(lam.rhs).max())
    with pytest.raises(ValueError):
        solver.Multiply(lam, x, x)                                       # x == y


def _long_row_ba():
    """3 cameras x (2 T + 37) landmarks, T the chunk length: camera 0 sees every landmark (a row of two full chunks and a
    ragged one), the others every third (short rows beside it)."""
    n_lm, dc, dp = 2 * MULTIPLY_CHUNK + 37, 6, 3
    ptr, brow = [0, 1, 2, 3], [0, 1, 2]
    for p in range(n_lm):
        brow += [0] + ([1] if p % 3 == 0 else []) + ([2] if p % 3 == 1 else []) + [3 + p]
        ptr.append(len(brow))
    cs = np.concatenate([np.arange(4) * dc, 3 * dc + np.arange(1, n_lm + 1) * dp]).astype(np.int64)
    brow = np.asarray(brow, dtype=np.int32)
    dims = np.diff(cs)
    cols = np.repeat(np.arange(3 + n_lm), np.diff(ptr))
    lam = synth.BlockSystem(cs, np.asarray(ptr, dtype=np.int64), brow, np.zeros(int((dims[brow] * dims[cols]).sum())),
                            np.zeros(int(cs[-1])), 3, "long_row")
    return _randomize(lam, 17)


def test_long_rows_are_cut_into_chunks():
    lam = _long_row_ba()
    assert MULTIPLY_LONG_ROW <= 2 * MULTIPLY_CHUNK + 38                  # row 0 (its diagonal block + every landmark) is a long row
    x = np.random.default_rng(7).standard_normal(lam.n_scalars)
    ref = lam.to_scipy() @ x
    solver = CLinearSolver_HIP()
    y = solver.Multiply(lam, x)
    # row 0 sums 6 + 3 (2 T + 37) products: the bound of n_terms eps |Lambda| |x|, which 1e-13 relative lies well above
    n_terms = 6 + 3 * (2 * MULTIPLY_CHUNK + 37)
    bound = n_terms * np.finfo(float).eps * (abs(lam.to_scipy()) @ np.abs(x)).max()
    print(f"long row: {n_terms} terms, abs error {np.abs(y - ref).max():.2e}, bound {bound:.2e}, rel-inf {rel_inf(y, ref):.2e}")
    assert np.abs(y - ref).max() <= bound and rel_inf(y, ref) < TOL
    assert np.array_equal(solver.Multiply(lam, x), y)
    short = CLinearSolver_HIP(multiply_long_row=1 << 20)                 # the same rows as short rows: another order of sums
    assert rel_inf(short.Multiply(lam, x), ref) < TOL


def test_forced_long_rows_on_a_golden_ba_system():
    lam = _load("ba_12x150_venice")
    x = np.random.default_rng(8).standard_normal(lam.n_scalars)
    ref = lam.to_scipy() @ x
    solver = CLinearSolver_HIP(multiply_long_row=4)                      # every row with more than 4 blocks in chunks of 4
    y = solver.Multiply(lam, x)
    assert rel_inf(y, ref) < TOL
    assert np.array_equal(solver.Multiply(lam, x), y)
    r = lam.rhs.copy()
    solver.Multiply(lam, x, r, alpha=-1.0, beta=1.0)                     # alpha / beta through the second pass as well
    assert np.abs(r - (lam.rhs - ref)).max() < TOL * max(np.abs(ref).max(), np.abs(lam.rhs).max())
    plain = CLinearSolver_HIP()
    plain.Multiply(lam, x)
    plain.set_option("multiply_long_row", 4)                             # the lists are rebuilt for the new threshold
    assert np.array_equal(plain.Multiply(lam, x), y)


def test_mixed_block_dimensions():
    """Poses of 6 and landmarks of 3 in one graph (the structure of test_assembly_gpu.test_two_edge_sets_accumulate)."""
    n_poses, n_lm = 400, 900
    rng = np.random.default_rng(8)
    dims = np.concatenate([np.full(n_poses, 6), np.full(n_lm, 3)])
    a0, a1 = np.arange(n_poses - 1), np.arange(1, n_poses)
    b0 = rng.integers(0, n_poses, 3 * n_lm)
    b1 = np.repeat(np.arange(n_lm), 3) + n_poses
    lam = _randomize(synth.structure_from_edges(dims, np.concatenate([a0, b0]), np.concatenate([a1, b1])), 9)
    x = rng.standard_normal(lam.n_scalars)
    y = CLinearSolver_HIP().Multiply(lam, x)
    assert rel_inf(y, lam.to_scipy() @ x) < TOL


@pytest.mark.parametrize("dims", [(11, 3), (9, 9)])
def test_block_columns_wider_than_eight_take_the_generic_path(dims):
    rng = np.random.default_rng(sum(dims))
    n = 60
    d = np.where(rng.random(n) < 0.4, dims[0], dims[1])
    a, b = rng.integers(0, n, 90), rng.integers(0, n, 90)
    v0 = np.concatenate([np.arange(n - 1), np.minimum(a, b)[a != b]])
    v1 = np.concatenate([np.arange(1, n), np.maximum(a, b)[a != b]])
    lam = _randomize(synth.structure_from_edges(d, v0, v1), 10)
    x = rng.standard_normal(lam.n_scalars)
    solver = CLinearSolver_HIP()
    y = solver.Multiply(lam, x)
    assert rel_inf(y, lam.to_scipy() @ x) < TOL
    assert np.array_equal(solver.Multiply(lam, x), y)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 100_003])
def test_dot_product(n):
    import torch
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    ad, bd = torch.tensor(a, device="cuda"), torch.tensor(b, device="cuda")
    out = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    solver = CLinearSolver_HIP()
    solver.dot_device(ad.data_ptr(), bd.data_ptr(), n, out.data_ptr())
    solver.dot_device(ad.data_ptr(), bd.data_ptr(), n, out.data_ptr() + 8)
    assert solver.sync()
    got = out.cpu().numpy()
    # any order of n products and n - 1 additions stays within n eps sum |a_i b_i| of the exact sum; numpy's is another such order
    bound = 2 * n * np.finfo(float).eps * np.abs(a * b).sum()
    assert abs(got[0] - np.dot(a, b)) <= bound
    assert got[0] == got[1]


def test_without_a_structure():
    import torch
    v = torch.zeros(8, dtype=torch.float64, device="cuda")
    w = torch.zeros(8, dtype=torch.float64, device="cuda")
    solver = CLinearSolver_HIP()
    with pytest.raises(ValueError):
        solver.multiply_device(v.data_ptr(), v.data_ptr(), w.data_ptr())
    assert "set_structure" in solver._error()
    assert hip_solver.ERR_INVALID == solver._lib.slampp_hip_multiply_device_async(solver._h, v.data_ptr(), v.data_ptr(), w.data_ptr(), 1.0, 0.0)
