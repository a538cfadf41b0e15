"""out = alpha P(a, b) + beta out on Lambda's block pattern (slampp_hip_pattern_outer / _device_async / _batch_device_async)
against torch_solve.pattern_outer_reference, element by element: every golden and dump system, block sizes whose pairs of
values straddle blocks, an odd number of values, a block column of width 11, a camera row of several hundred blocks,
batches with even and odd strides, bit-reproducibility, the adjoint identity against the product, and the refusals."""
import numpy as np
import pytest
import torch

from slam_plus_plus_amd import synth, hip_solver
from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP, CLinearSolver_Schur_HIP
from slam_plus_plus_amd.torch_solve import pattern_outer_reference
from golden_util import golden_names, dump_names, load_golden, load_dump

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
SYSTEMS = golden_names() + dump_names()


def _load(name):
    return load_dump(name)[0] if name.startswith("dump_") else load_golden(name)[0]


def _mixed_6_and_3():
    """Poses of 6 and landmarks of 3 in one graph: blocks of 36, 18 and 9 values (9 is odd: 16-byte stores straddle blocks)."""
    n_poses, n_lm = 40, 90
    rng = np.random.default_rng(8)
    dims = np.concatenate([np.full(n_poses, 6), np.full(n_lm, 3)])
    a0, a1 = np.arange(n_poses - 1), np.arange(1, n_poses)
    b0, b1 = rng.integers(0, n_poses, 3 * n_lm), np.repeat(np.arange(n_lm), 3) + n_poses
    return synth.structure_from_edges(dims, np.concatenate([a0, b0]), np.concatenate([a1, b1]))


def _odd_number_of_values():
    """A chain of 21 blocks of 3: 41 blocks of 9 values, 369 in all (three chunks, the last one ragged and its last pair single)."""
    lam = synth.structure_from_edges(np.full(21, 3), np.arange(20), np.arange(1, 21))
    assert lam.values.shape[0] == 369
    return lam


def _one_column_of_11():
    rng = np.random.default_rng(11)
    n = 30
    dims = np.full(n, 7)
    dims[13] = 11
    a, b = rng.integers(0, n, 40), rng.integers(0, n, 40)
    return synth.structure_from_edges(dims, np.concatenate([np.arange(n - 1), np.minimum(a, b)[a != b]]),
                                      np.concatenate([np.arange(1, n), np.maximum(a, b)[a != b]]))


def _long_camera_row():
    """3 cameras x 550 landmarks, camera 0 sees every landmark (a row of 550 blocks of 18 values: seven blocks per chunk),
    the others every third; the number of values is no multiple of the chunk."""
    n_lm, dc, dp = 550, 6, 3
    ptr, brow = [0, 1, 2, 3], [0, 1, 2]
    for p in range(n_lm):
        brow += [0] + ([1] if p % 3 == 0 else []) + ([2] if p % 3 == 1 else []) + [3 + p]
        ptr.append(len(brow))
    cs = np.concatenate([np.arange(4) * dc, 3 * dc + np.arange(1, n_lm + 1) * dp]).astype(np.int64)
    brow = np.asarray(brow, dtype=np.int32)
    dims = np.diff(cs)
    cols = np.repeat(np.arange(3 + n_lm), np.diff(ptr))
    lam = synth.BlockSystem(cs, np.asarray(ptr, dtype=np.int64), brow, np.zeros(int((dims[brow] * dims[cols]).sum())),
                            np.zeros(int(cs[-1])), 3, "long_camera_row")
    assert lam.values.shape[0] % 128 != 0
    return lam


STRUCTURES = {"mixed_6_and_3": _mixed_6_and_3, "odd_number_of_values": _odd_number_of_values,
              "one_column_of_11": _one_column_of_11, "long_camera_row": _long_camera_row}


def _get(name):
    return STRUCTURES[name]() if name in STRUCTURES else _load(name)


def _dev(a):
    return torch.tensor(a, dtype=torch.float64, device="cuda")


def _vectors(lam, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(lam.n_scalars), rng.standard_normal(lam.n_scalars)


def _assert_within_bound(got, lam, a, b, alpha, out0=None, beta=0.0):
    """Element by element: two products and one add (fused or not), the scaling by alpha, and for beta != 0 one more
    multiply-add -- within 4 eps |alpha| (|a_r||b_c|^T + |b_r||a_c|^T) (+ 4 eps |out|) of the reference."""
    ref = pattern_outer_reference(lam, a, b, alpha)
    bound = 4 * EPS * abs(alpha) * pattern_outer_reference(lam, np.abs(a), np.abs(b))
    if out0 is not None:
        ref = ref + beta * out0
        bound = bound + 4 * EPS * np.abs(out0)
    excess = np.abs(got - ref) - bound
    print(f"{lam.name}: alpha {alpha} beta {beta}: max |error| {np.abs(got - ref).max():.2e}, max bound {bound.max():.2e}, "
          f"worst error / bound {np.max(np.abs(got - ref) / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(np.isfinite(got)) and excess.max() <= 0


@pytest.mark.parametrize("name", SYSTEMS + sorted(STRUCTURES))
def test_outer_product_matches_the_reference_element_by_element(name):
    lam = _get(name)
    a, b = _vectors(lam, 21)
    n_values = lam.values.shape[0]
    solver = CLinearSolver_HIP()
    out = solver.Pattern_Outer(lam, a, b)                                # the host entry point
    assert out.shape == (n_values,)
    _assert_within_bound(out, lam, a, b, 1.0)
    # the device entry point: beta = 0 does not read a NaN-filled out; the same bits as the host one, twice
    ad, bd = _dev(a), _dev(b)
    od = torch.full((n_values,), float("nan"), dtype=torch.float64, device="cuda")
    solver.pattern_outer_device(ad.data_ptr(), bd.data_ptr(), od.data_ptr())
    assert solver.sync()
    assert not torch.isnan(od).any() and np.array_equal(od.cpu().numpy(), out)
    od2 = torch.full((n_values,), float("nan"), dtype=torch.float64, device="cuda")
    solver.pattern_outer_device(ad.data_ptr(), bd.data_ptr(), od2.data_ptr())
    assert solver.sync() and torch.equal(od, od2)
    # an out that is not 16-byte aligned takes 8-byte stores: the same bits
    shifted = torch.full((n_values + 1,), float("nan"), dtype=torch.float64, device="cuda")
    assert shifted.data_ptr() % 16 == 0
    solver.pattern_outer_device(ad.data_ptr(), bd.data_ptr(), shifted.data_ptr() + 8)
    assert solver.sync() and torch.equal(shifted[1:], od) and bool(torch.isnan(shifted[0]))
    # alpha = -1, beta = 1 on a random out, aligned and not
    out0 = np.random.default_rng(22).standard_normal(n_values)
    acc = out0.copy()
    assert solver.Pattern_Outer(lam, a, b, acc, alpha=-1.0, beta=1.0) is acc
    _assert_within_bound(acc, lam, a, b, -1.0, out0, 1.0)
    shifted[1:] = _dev(out0)
    solver.pattern_outer_device(ad.data_ptr(), bd.data_ptr(), shifted.data_ptr() + 8, -1.0, 1.0)
    assert solver.sync() and np.array_equal(shifted[1:].cpu().numpy(), acc)
    # another alpha
    _assert_within_bound(solver.Pattern_Outer(lam, a, b, alpha=2.5), lam, a, b, 2.5)


@pytest.mark.parametrize("name", ["chain6_n60", "ba_12x150_venice", "mixed_6_and_3", "one_column_of_11", "long_camera_row"])
@pytest.mark.parametrize("schur", [False, True])
def test_adjoint_of_the_product(name, schur):
    """<v, P(a, b)> = a^T M(v) b with the library's own product and dot product, in either mode (no analysis)."""
    lam = _get(name)
    a, b = _vectors(lam, 23)
    v = np.random.default_rng(24).standard_normal(lam.values.shape[0])
    lam.values = v
    solver = (CLinearSolver_Schur_HIP if schur else CLinearSolver_HIP)()
    solver._set_structure(lam)
    vd, ad, bd = _dev(v), _dev(a), _dev(b)
    P = torch.empty_like(vd)
    y = torch.empty_like(ad)
    dots = torch.zeros(2, dtype=torch.float64, device="cuda")
    solver.pattern_outer_device(ad.data_ptr(), bd.data_ptr(), P.data_ptr())
    solver.dot_device(vd.data_ptr(), P.data_ptr(), v.shape[0], dots.data_ptr())
    solver.multiply_device(vd.data_ptr(), bd.data_ptr(), y.data_ptr())
    solver.dot_device(ad.data_ptr(), y.data_ptr(), lam.n_scalars, dots.data_ptr() + 8)
    assert solver.sync()
    lhs, rhs = dots.cpu().numpy()
    terms = float(np.abs(v) @ pattern_outer_reference(lam, np.abs(a), np.abs(b)))
    print(f"{name}: <v, P(a, b)> = {lhs:.15e}, a^T M(v) b = {rhs:.15e}, sum |terms| = {terms:.3e}")
    assert abs(lhs - rhs) <= 1e-12 * terms


@pytest.mark.parametrize("name", ["chain6_n60", "chain7_n40", "mixed_6_and_3"])
@pytest.mark.parametrize("out_pad", [2, 3], ids=["even_strides", "odd_out_stride"])
def test_batch_of_three_equals_the_single_calls(name, out_pad):
    lam = _get(name)
    n, n_values = lam.n_scalars, lam.values.shape[0]
    rng = np.random.default_rng(25)
    a, b = _dev(rng.standard_normal((3, n))), _dev(rng.standard_normal((3, n + 2)))[:, :n]
    n_out_stride = n_values + out_pad + (n_values % 2)                   # even for out_pad = 2, odd for 3
    assert n_out_stride % 2 == out_pad % 2
    out = torch.full((3, n_out_stride), float("nan"), dtype=torch.float64, device="cuda")
    solver = CLinearSolver_HIP()
    solver._set_structure(lam)
    solver.pattern_outer_batch_device(3, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0), -1.0, 0.0)
    single = torch.empty((3, n_values), dtype=torch.float64, device="cuda")
    for m in range(3):
        solver.pattern_outer_device(a[m].data_ptr(), b[m].data_ptr(), single[m].data_ptr(), -1.0, 0.0)
    assert solver.sync()
    assert torch.equal(out[:, :n_values], single)
    assert bool(torch.isnan(out[:, n_values:]).all())                    # nothing is written between the members
    _assert_within_bound(single[1].cpu().numpy(), lam, a[1].cpu().numpy(), b[1].cpu().numpy(), -1.0)
    # beta through the batch
    acc = torch.ones_like(out)
    solver.pattern_outer_batch_device(3, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), acc.data_ptr(), acc.stride(0), 1.0, 1.0)
    assert solver.sync()
    assert torch.equal(acc[:, :n_values], 1.0 - single) and bool((acc[:, n_values:] == 1.0).all())


def test_refusals():
    lam = _load("chain6_n60")
    n, n_values = lam.n_scalars, lam.values.shape[0]
    buf = torch.zeros(2 * n + n_values, dtype=torch.float64, device="cuda")
    a, b, out = buf[:n], buf[n:2 * n], buf[2 * n:]
    solver = CLinearSolver_HIP()
    lib, h = solver._lib, solver._h
    INVALID, UNSUPPORTED = hip_solver.ERR_INVALID, hip_solver.ERR_UNSUPPORTED
    assert lib.slampp_hip_pattern_outer_device_async(h, a.data_ptr(), b.data_ptr(), out.data_ptr(), 1.0, 0.0) == INVALID
    assert "set_structure" in solver._error()                             # no structure
    host = np.zeros(n)
    assert lib.slampp_hip_pattern_outer(h, host.ctypes.data, host.ctypes.data, np.zeros(n_values).ctypes.data, 1.0, 0.0) == INVALID
    solver._set_structure(lam)
    assert lib.slampp_hip_pattern_outer_device_async(h, a.data_ptr(), b.data_ptr(), out.data_ptr(), 1.0, 0.0) == hip_solver.OK
    assert lib.slampp_hip_pattern_outer_device_async(h, a.data_ptr(), a.data_ptr(), out.data_ptr(), 1.0, 0.0) == hip_solver.OK   # a == b is fine
    for args in [(None, b.data_ptr(), out.data_ptr()), (a.data_ptr(), None, out.data_ptr()), (a.data_ptr(), b.data_ptr(), None)]:
        assert lib.slampp_hip_pattern_outer_device_async(h, *args, 1.0, 0.0) == INVALID                                            # null pointer
    assert lib.slampp_hip_pattern_outer(h, None, host.ctypes.data, np.zeros(n_values).ctypes.data, 1.0, 0.0) == INVALID
    for n_batch in (0, -1, 65):
        assert lib.slampp_hip_pattern_outer_batch_device_async(h, n_batch, a.data_ptr(), n, b.data_ptr(), n, out.data_ptr(),
                                                               n_values, 1.0, 0.0) == INVALID
    big = torch.zeros(2 * (2 * n + n_values), dtype=torch.float64, device="cuda")
    for strides in [(n - 1, n, n_values), (n, n - 1, n_values), (n, n, n_values - 1)]:                                            # a stride below a member
        assert lib.slampp_hip_pattern_outer_batch_device_async(h, 2, big.data_ptr(), strides[0], big.data_ptr() + 8 * 2 * n, strides[1],
                                                               big.data_ptr() + 8 * 4 * n, strides[2], 1.0, 0.0) == INVALID
    # out overlapping a or b: its first value is the last entry of b; it begins inside a
    assert lib.slampp_hip_pattern_outer_device_async(h, a.data_ptr(), b.data_ptr(), out.data_ptr() - 8, 1.0, 0.0) == INVALID
    assert lib.slampp_hip_pattern_outer_device_async(h, a.data_ptr(), b.data_ptr(), a.data_ptr() + 8 * (n - 1), 1.0, 0.0) == INVALID
    assert "overlaps" in solver._error()
    with pytest.raises(ValueError):
        solver.pattern_outer_device(a.data_ptr(), b.data_ptr(), a.data_ptr())
    assert solver.sync()
    # a handle that solves with landmark shards
    ba = _load("ba_10x120_band")
    group = CLinearSolver_Schur_HIP(devices=[0, 0])
    group.SymbolicDecomposition_Blocky(ba)
    v = torch.zeros(2 * ba.n_scalars + ba.values.shape[0], dtype=torch.float64, device="cuda")
    args = (v.data_ptr(), v.data_ptr() + 8 * ba.n_scalars, v.data_ptr() + 16 * ba.n_scalars)
    assert group._lib.slampp_hip_pattern_outer_device_async(group._h, *args, 1.0, 0.0) == UNSUPPORTED
    assert group._lib.slampp_hip_pattern_outer_batch_device_async(group._h, 1, args[0], 0, args[1], 0, args[2], 0, 1.0, 0.0) == UNSUPPORTED
    with pytest.raises(NotImplementedError):
        group.pattern_outer_device(*args)
