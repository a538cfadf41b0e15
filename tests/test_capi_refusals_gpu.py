"""The C entry points' refusals and the handle's factor state, as the callers of include/slampp_hip.h see them: for every
host entry point that makes a round trip to the device, and for every _device_async twin the Python module declares, each
refusal it can give (exact status code, exact slampp_hip_last_error string); after every call that installs or drops a
factor, whether a re-solve and a values = NULL covariance call are accepted; and the grouping of block columns into passes
of at most 48 scalar columns, bitwise against the same columns asked for one at a time."""
import ctypes as C

import numpy as np
import pytest
import torch

from slam_plus_plus_amd import synth
from slam_plus_plus_amd.hip_solver import (CLinearSolver_HIP, CLinearSolver_Schur_HIP, _ptr, OK, NOT_POSDEF, ERR_INVALID,
                                           ERR_UNSUPPORTED)

pytestmark = pytest.mark.gpu
COV_K_PASS = 48                                                        # csrc/covariance.h

NO_KEPT = (": no kept factor of the reduced camera system: set the option schur_keep (or schur_incremental) before analyze "
           "and solve, or call a Schur covariance entry point; anything that factors or fails to since ends its validity")
NO_REUSE = (": no factorization to reuse (values = NULL): none was left by a Schur covariance call, another factorization ran "
            "since, or it was not positive definite")
SHARDS = ": not for a handle that solves with landmark shards or over several devices"
SPARSE_ONLY = ": sparse mode only (Schur mode: slampp_hip_schur_marginals)"
SCHUR_ONLY = ": needs the Schur mode (sparse mode: slampp_hip_marginals_pattern, slampp_hip_marginal_columns)"
CAMERAS = ": needs the Schur mode (cameras and landmarks)"
ALLREDUCE = ": not with landmark shards (an all-reduce callback is set)"
X_IS_Y = "multiply: x and y must be different vectors (every row of y reads all of x)"
COLS_NO_REUSE = "marginal_columns: no valid factorization to reuse (values = NULL)"


def dev(n):
    return torch.zeros(int(n), dtype=torch.float64, device="cuda")


class Handle:
    """A solver, its system, and host and device arrays big enough for every entry point's arguments."""

    def __init__(self, solver, lam, analyze=True, structure=True):
        self.s, self.lam, self.lib, self.h = solver, lam, solver._lib, solver._h
        if analyze:
            solver.SymbolicDecomposition_Blocky(lam)
        elif structure:
            solver._set_structure(lam)
        n, nv = int(lam.n_scalars), int(lam.values.shape[0])
        self.vals = np.ascontiguousarray(lam.values, dtype=np.float64)
        self.rhs = np.ascontiguousarray(lam.rhs, dtype=np.float64).copy()
        self.x, self.y = np.zeros(n), np.zeros(n)
        self.out = np.zeros(max(nv, n * COV_K_PASS))                   # any covariance result of up to one pass
        self.cols = np.array([1, 0], dtype=np.int64)
        self.t_vals = torch.from_numpy(self.vals).cuda()
        self.t_rhs, self.t_x, self.t_y, self.t_out = dev(n), dev(n), dev(n), dev(self.out.shape[0])
        self.dv, self.dr, self.dx, self.dy, self.do = (t.data_ptr() for t in (self.t_vals, self.t_rhs, self.t_x, self.t_y, self.t_out))
        self.hv, self.hr, self.hx, self.hy, self.ho, self.hc = (_ptr(a) for a in (self.vals, self.rhs, self.x, self.y, self.out, self.cols))

    def refused(self, rc, code, msg):
        assert (rc, self.s._error()) == (code, msg)

    def ok(self, rc):
        assert rc == OK, (rc, self.s._error())

    def factor_solve(self, vals=None):
        rhs = self.rhs.copy()
        return self.lib.slampp_hip_factor_solve(self.h, _ptr(self.vals if vals is None else vals), _ptr(rhs), None)

    # the probes of the state table
    def again(self):
        return self.lib.slampp_hip_solve_again_device_async(self.h, self.dr)

    def cols_null(self):
        return self.lib.slampp_hip_marginal_columns(self.h, None, 2, self.hc, self.ho)

    def pattern_null(self):
        return self.lib.slampp_hip_schur_marginals_pattern(self.h, None, self.ho)

    def sync(self):
        return self.lib.slampp_hip_sync(self.h)

    def set_structure(self):
        lam = self.lam
        cs, bp = (np.ascontiguousarray(a, dtype=np.int64) for a in (lam.cumsum, lam.bcol_ptr))
        br = np.ascontiguousarray(lam.brow_idx, dtype=np.int32)
        return self.lib.slampp_hip_set_structure(self.h, lam.n_bcols, _ptr(cs), _ptr(bp), _ptr(br))


@pytest.fixture(scope="module")
def chain():
    return synth.pose_chain(n=40, d=6, seed=2)


@pytest.fixture(scope="module")
def ba():
    return synth.ba(8, 200, seed=1)


# ---- refusals ----

def test_no_analyze(chain):
    L = CLinearSolver_HIP()._lib
    bare = Handle(CLinearSolver_HIP(), chain, analyze=False, structure=False)
    a = Handle(CLinearSolver_HIP(), chain, analyze=False)
    for g in (bare, a):
        h = g.h
        g.refused(L.slampp_hip_marginals(h, g.hv, g.ho), ERR_INVALID, "marginals: analyze was not called")
        g.refused(L.slampp_hip_marginals_device_async(h, g.dv, g.do), ERR_INVALID, "marginals: analyze was not called")
        g.refused(L.slampp_hip_marginals_pattern(h, g.hv, g.ho), ERR_INVALID, "marginals_pattern: analyze was not called")
        g.refused(L.slampp_hip_marginals_pattern_device_async(h, g.dv, g.do), ERR_INVALID, "marginals_pattern: analyze was not called")
        g.refused(L.slampp_hip_marginal_columns(h, g.hv, 2, g.hc, g.ho), ERR_INVALID, "marginal_columns: analyze was not called")
        g.refused(L.slampp_hip_marginal_columns_device_async(h, g.dv, 2, g.hc, g.do), ERR_INVALID, "marginal_columns: analyze was not called")
        g.refused(L.slampp_hip_schur_marginals(h, g.hv, g.ho, None), ERR_INVALID, "schur_marginals: analyze was not called")
        g.refused(L.slampp_hip_schur_marginals_device_async(h, g.dv, g.do, None), ERR_INVALID, "schur_marginals: analyze was not called")
        g.refused(L.slampp_hip_schur_marginals_pattern(h, g.hv, g.ho), ERR_INVALID, "schur_marginals_pattern: analyze was not called")
        g.refused(L.slampp_hip_schur_marginals_pattern_device_async(h, g.dv, g.do), ERR_INVALID, "schur_marginals_pattern: analyze was not called")
        g.refused(L.slampp_hip_schur_marginal_columns(h, g.hv, 2, g.hc, g.ho), ERR_INVALID, "schur_marginal_columns: analyze was not called")
        g.refused(L.slampp_hip_schur_marginal_columns_device_async(h, g.dv, 2, g.hc, g.do), ERR_INVALID, "schur_marginal_columns: analyze was not called")
        g.refused(L.slampp_hip_solve_marginal_poses(h, g.hv, g.hr), ERR_INVALID, "solve_marginal_poses: analyze was not called")
        g.refused(L.slampp_hip_solve_marginal_poses_device_async(h, g.dv, g.dr), ERR_INVALID, "solve_marginal_poses: analyze was not called")
        g.refused(L.slampp_hip_factorize(h, g.hv, g.ho), ERR_INVALID, "factorize: analyze was not called")
        g.refused(L.slampp_hip_solve_again(h, g.hr), ERR_INVALID, "solve_again: no valid factorization")
        g.refused(L.slampp_hip_solve_again_device_async(h, g.dr), ERR_INVALID, "solve_again: no valid factorization (analyze was not called)")
    # the product needs the structure only; the refinement asks for it first, then for a factor
    g = bare
    g.refused(L.slampp_hip_multiply(g.h, g.hv, g.hx, g.hy, 1.0, 0.0), ERR_INVALID, "multiply: set_structure was not called")
    g.refused(L.slampp_hip_multiply_device_async(g.h, g.dv, g.dx, g.dy, 1.0, 0.0), ERR_INVALID, "multiply: set_structure was not called")
    g.refused(L.slampp_hip_refine(g.h, g.hv, g.hr, g.hx, 2, None), ERR_INVALID, "refine: set_structure was not called")
    g.refused(L.slampp_hip_refine_device_async(g.h, g.dv, g.dr, g.dx, 2, None), ERR_INVALID, "refine: set_structure was not called")
    g = a
    g.ok(L.slampp_hip_multiply(g.h, g.hv, g.hx, g.hy, 1.0, 0.0))
    g.ok(L.slampp_hip_multiply_device_async(g.h, g.dv, g.dx, g.dy, 1.0, 0.0))
    g.refused(L.slampp_hip_refine(g.h, g.hv, g.hr, g.hx, 2, None), ERR_INVALID, "refine: no valid factorization (analyze was not called)")
    g.refused(L.slampp_hip_refine_device_async(g.h, g.dv, g.dr, g.dx, 2, None), ERR_INVALID, "refine: no valid factorization (analyze was not called)")
    # two conditions at once: every entry point asks for the analysis before it looks at its pointers
    g.refused(L.slampp_hip_marginals(g.h, None, None), ERR_INVALID, "marginals: analyze was not called")
    g.refused(L.slampp_hip_factorize(g.h, None, None), ERR_INVALID, "factorize: analyze was not called")
    g.refused(L.slampp_hip_solve_again(g.h, None), ERR_INVALID, "solve_again: no valid factorization")


def test_sparse_handle_refusals(chain):
    g = Handle(CLinearSolver_HIP(), chain)
    L, h = g.lib, g.h
    # wrong mode (the host entry points upload, their device twins refuse)
    for rc in (L.slampp_hip_schur_marginals(h, g.hv, g.ho, None), L.slampp_hip_schur_marginals_device_async(h, g.dv, g.do, None)):
        g.refused(rc, ERR_UNSUPPORTED, "schur_marginals" + CAMERAS)
    g.refused(L.slampp_hip_schur_marginals_pattern(h, g.hv, g.ho), ERR_UNSUPPORTED, "schur_marginals_pattern" + SCHUR_ONLY)
    g.refused(L.slampp_hip_schur_marginals_pattern_device_async(h, g.dv, g.do), ERR_UNSUPPORTED, "schur_marginals_pattern" + SCHUR_ONLY)
    g.refused(L.slampp_hip_schur_marginals_pattern(h, None, None), ERR_UNSUPPORTED, "schur_marginals_pattern" + SCHUR_ONLY)   # (before values = NULL, before the null output)
    g.refused(L.slampp_hip_schur_marginal_columns(h, g.hv, 2, g.hc, g.ho), ERR_UNSUPPORTED, "schur_marginal_columns" + SCHUR_ONLY)
    g.refused(L.slampp_hip_schur_marginal_columns_device_async(h, g.dv, 2, g.hc, g.do), ERR_UNSUPPORTED, "schur_marginal_columns" + SCHUR_ONLY)
    g.refused(L.slampp_hip_solve_marginal_poses(h, g.hv, g.hr), ERR_UNSUPPORTED, "solve_marginal_poses" + CAMERAS)
    g.refused(L.slampp_hip_solve_marginal_poses_device_async(h, g.dv, g.dr), ERR_UNSUPPORTED, "solve_marginal_poses" + CAMERAS)
    # ... two conditions at once: the host entry point meets the null pointer first, its device twin the mode
    g.refused(L.slampp_hip_solve_marginal_poses(h, g.hv, None), ERR_INVALID, "solve_marginal_poses: null pointer")
    g.refused(L.slampp_hip_solve_marginal_poses_device_async(h, g.dv, None), ERR_UNSUPPORTED, "solve_marginal_poses" + CAMERAS)
    g.refused(L.slampp_hip_schur_marginals(h, None, g.ho, None), ERR_UNSUPPORTED, "schur_marginals" + CAMERAS)
    # null pointers
    for rc in (L.slampp_hip_marginals(h, None, g.ho), L.slampp_hip_marginals(h, g.hv, None),
               L.slampp_hip_marginals_device_async(h, None, g.do), L.slampp_hip_marginals_device_async(h, g.dv, None)):
        g.refused(rc, ERR_INVALID, "marginals: null pointer")
    for rc in (L.slampp_hip_marginals_pattern(h, None, g.ho), L.slampp_hip_marginals_pattern(h, g.hv, None),
               L.slampp_hip_marginals_pattern_device_async(h, None, g.do), L.slampp_hip_marginals_pattern_device_async(h, g.dv, None)):
        g.refused(rc, ERR_INVALID, "marginals_pattern: null pointer")
    g.refused(L.slampp_hip_marginal_columns(h, g.hv, 2, g.hc, None), ERR_INVALID, "marginal_columns: null pointer")
    g.refused(L.slampp_hip_marginal_columns_device_async(h, g.dv, 2, g.hc, None), ERR_INVALID, "marginal_columns: null pointer")
    for rc in (L.slampp_hip_factorize(h, None, g.ho), L.slampp_hip_factorize(h, g.hv, None)):
        g.refused(rc, ERR_INVALID, "factorize: null pointer")
    for rc in (L.slampp_hip_multiply(h, None, g.hx, g.hy, 1.0, 0.0), L.slampp_hip_multiply(h, g.hv, None, g.hy, 1.0, 0.0),
               L.slampp_hip_multiply(h, g.hv, g.hx, None, 1.0, 0.0), L.slampp_hip_multiply(h, g.hv, None, None, 1.0, 0.0),   # (null before x == y)
               L.slampp_hip_multiply_device_async(h, None, g.dx, g.dy, 1.0, 0.0), L.slampp_hip_multiply_device_async(h, g.dv, None, g.dy, 1.0, 0.0),
               L.slampp_hip_multiply_device_async(h, g.dv, g.dx, None, 1.0, 0.0)):
        g.refused(rc, ERR_INVALID, "multiply: null pointer")
    g.refused(L.slampp_hip_multiply(h, g.hv, g.hx, g.hx, 1.0, 0.0), ERR_INVALID, X_IS_Y)
    g.refused(L.slampp_hip_multiply_device_async(h, g.dv, g.dx, g.dx, 1.0, 0.0), ERR_INVALID, X_IS_Y)
    # the column list (its checks come behind the null output and before values = NULL)
    n = chain.n_bcols
    for fn, vals, out in ((L.slampp_hip_marginal_columns, g.hv, g.ho), (L.slampp_hip_marginal_columns_device_async, g.dv, g.do)):
        for null_vals in (False, True):
            v = None if null_vals else vals
            g.refused(fn(h, v, 0, g.hc, out), ERR_INVALID, "marginal_columns: no columns")
            g.refused(fn(h, v, 2, None, out), ERR_INVALID, "marginal_columns: no columns")
            for bad in ([n], [-1], [3, n], [0, -1]):
                c = np.array(bad, dtype=np.int64)
                g.refused(fn(h, v, len(bad), _ptr(c), out), ERR_INVALID, "marginal_columns: block column index out of range")
            c = np.array([3, 5, 3], dtype=np.int64)
            g.refused(fn(h, v, 3, _ptr(c), out), ERR_INVALID, "marginal_columns: a block column is listed twice")
            g.refused(fn(h, v, 0, g.hc, None), ERR_INVALID, "marginal_columns: null pointer")
    # no factor yet
    g.refused(g.cols_null(), ERR_INVALID, COLS_NO_REUSE)
    g.refused(L.slampp_hip_marginal_columns_device_async(h, None, 2, g.hc, g.do), ERR_INVALID, COLS_NO_REUSE)
    g.refused(L.slampp_hip_solve_again(h, g.hr), ERR_INVALID, "solve_again: no valid factorization")
    g.refused(L.slampp_hip_solve_again(h, None), ERR_INVALID, "solve_again: no valid factorization")
    g.refused(g.again(), ERR_INVALID, "solve_again: no valid factorization")
    g.refused(L.slampp_hip_solve_again_device_async(h, None), ERR_INVALID, "solve_again: no valid factorization")
    g.refused(L.slampp_hip_refine(h, g.hv, g.hr, g.hx, 2, None), ERR_INVALID, "refine: no valid factorization")
    g.refused(L.slampp_hip_refine(h, None, g.hr, g.hx, 0, None), ERR_INVALID, "refine: no valid factorization")
    g.refused(L.slampp_hip_refine_device_async(h, g.dv, g.dr, g.dx, 2, None), ERR_INVALID, "refine: no valid factorization")
    # with a factor: the pointers, the steps, eta == x
    g.ok(g.factor_solve())
    g.refused(L.slampp_hip_solve_again(h, None), ERR_INVALID, "solve_again: null pointer")
    g.refused(L.slampp_hip_solve_again_device_async(h, None), ERR_INVALID, "solve_again: null pointer")
    for rc in (L.slampp_hip_refine(h, None, g.hr, g.hx, 2, None), L.slampp_hip_refine(h, g.hv, None, g.hx, 2, None),
               L.slampp_hip_refine(h, g.hv, g.hr, None, 0, None),                                                    # (null before the steps)
               L.slampp_hip_refine_device_async(h, None, g.dr, g.dx, 2, None), L.slampp_hip_refine_device_async(h, g.dv, None, g.dx, 2, None),
               L.slampp_hip_refine_device_async(h, g.dv, g.dr, None, 9, None)):
        g.refused(rc, ERR_INVALID, "refine: null pointer")
    for steps in (0, 9, -1):
        g.refused(L.slampp_hip_refine(h, g.hv, g.hr, g.hx, steps, None), ERR_INVALID, "refine: between 1 and 8 steps")
        g.refused(L.slampp_hip_refine_device_async(h, g.dv, g.dr, g.dx, steps, None), ERR_INVALID, "refine: between 1 and 8 steps")
        g.refused(L.slampp_hip_refine_device_async(h, g.dv, g.dx, g.dx, steps, None), ERR_INVALID, "refine: between 1 and 8 steps")   # (the steps before eta == x)
    g.refused(L.slampp_hip_refine_device_async(h, g.dv, g.dx, g.dx, 2, None), ERR_INVALID, "refine: eta and x must be different vectors")
    g.ok(L.slampp_hip_refine(h, g.hv, g.hx, g.hx, 1, None))          # (the host entry point uploads eta and x into arrays of its own)
    g.ok(L.slampp_hip_refine(h, g.hv, g.hr, g.hx, 8, None))
    g.ok(L.slampp_hip_refine_device_async(h, g.dv, g.dr, g.dx, 1, None))
    g.ok(g.sync())


def test_schur_handle_refusals(ba):
    g = Handle(CLinearSolver_Schur_HIP(), ba)
    L, h = g.lib, g.h
    # wrong mode
    g.refused(L.slampp_hip_marginals(h, g.hv, g.ho), ERR_UNSUPPORTED, "marginals" + SPARSE_ONLY)
    g.refused(L.slampp_hip_marginals_device_async(h, g.dv, g.do), ERR_UNSUPPORTED, "marginals" + SPARSE_ONLY)
    # ... two conditions at once: the host entry point meets the null pointer first, its device twin the mode
    g.refused(L.slampp_hip_marginals(h, g.hv, None), ERR_INVALID, "marginals: null pointer")
    g.refused(L.slampp_hip_marginals_device_async(h, g.dv, None), ERR_UNSUPPORTED, "marginals" + SPARSE_ONLY)
    for rc in (L.slampp_hip_marginals_pattern(h, g.hv, g.ho), L.slampp_hip_marginals_pattern(h, None, None),
               L.slampp_hip_marginals_pattern_device_async(h, g.dv, g.do), L.slampp_hip_marginals_pattern_device_async(h, None, None)):
        g.refused(rc, ERR_UNSUPPORTED, "marginals_pattern" + SPARSE_ONLY)
    for rc in (L.slampp_hip_marginal_columns(h, g.hv, 2, g.hc, g.ho), L.slampp_hip_marginal_columns(h, None, 0, None, None),
               L.slampp_hip_marginal_columns_device_async(h, g.dv, 2, g.hc, g.do)):
        g.refused(rc, ERR_UNSUPPORTED, "marginal_columns" + SPARSE_ONLY)
    g.refused(L.slampp_hip_factorize(h, g.hv, g.ho), ERR_UNSUPPORTED, "factorize: the sparse mode only")
    g.refused(L.slampp_hip_factorize(h, None, None), ERR_UNSUPPORTED, "factorize: the sparse mode only")
    # null pointers
    for rc in (L.slampp_hip_schur_marginals(h, None, g.ho, g.ho), L.slampp_hip_schur_marginals(h, g.hv, None, None),
               L.slampp_hip_schur_marginals_device_async(h, None, g.do, g.do), L.slampp_hip_schur_marginals_device_async(h, g.dv, None, None)):
        g.refused(rc, ERR_INVALID, "schur_marginals: null pointer")
    g.refused(L.slampp_hip_schur_marginals_pattern(h, g.hv, None), ERR_INVALID, "schur_marginals_pattern: null pointer")
    g.refused(L.slampp_hip_schur_marginals_pattern_device_async(h, g.dv, None), ERR_INVALID, "schur_marginals_pattern: null pointer")
    g.refused(L.slampp_hip_schur_marginal_columns(h, g.hv, 2, g.hc, None), ERR_INVALID, "schur_marginal_columns: null pointer")
    g.refused(L.slampp_hip_schur_marginal_columns_device_async(h, g.dv, 2, g.hc, None), ERR_INVALID, "schur_marginal_columns: null pointer")
    for rc in (L.slampp_hip_solve_marginal_poses(h, None, g.hr), L.slampp_hip_solve_marginal_poses(h, g.hv, None),
               L.slampp_hip_solve_marginal_poses_device_async(h, None, g.dr), L.slampp_hip_solve_marginal_poses_device_async(h, g.dv, None)):
        g.refused(rc, ERR_INVALID, "solve_marginal_poses: null pointer")
    # the column list
    n = ba.n_bcols
    for fn, vals, out in ((L.slampp_hip_schur_marginal_columns, g.hv, g.ho), (L.slampp_hip_schur_marginal_columns_device_async, g.dv, g.do)):
        g.refused(fn(h, vals, 0, g.hc, out), ERR_INVALID, "marginal_columns: no columns")
        g.refused(fn(h, vals, 2, None, out), ERR_INVALID, "marginal_columns: no columns")
        for bad in ([n], [-1], [3, n]):
            c = np.array(bad, dtype=np.int64)
            g.refused(fn(h, vals, len(bad), _ptr(c), out), ERR_INVALID, "marginal_columns: block column index out of range")
        c = np.array([n - 1, 5, n - 1], dtype=np.int64)
        g.refused(fn(h, vals, 3, _ptr(c), out), ERR_INVALID, "marginal_columns: a block column is listed twice")
        # values = NULL with nothing to reuse: before the null output and the column list
        g.refused(fn(h, None, 0, None, None), ERR_INVALID, "schur_marginal_columns" + NO_REUSE)
        g.refused(fn(h, None, 2, g.hc, out), ERR_INVALID, "schur_marginal_columns" + NO_REUSE)
    g.refused(g.pattern_null(), ERR_INVALID, "schur_marginals_pattern" + NO_REUSE)
    g.refused(L.slampp_hip_schur_marginals_pattern(h, None, None), ERR_INVALID, "schur_marginals_pattern" + NO_REUSE)
    g.refused(L.slampp_hip_schur_marginals_pattern_device_async(h, None, g.do), ERR_INVALID, "schur_marginals_pattern" + NO_REUSE)
    # no kept factor
    g.refused(g.again(), ERR_INVALID, "solve_again" + NO_KEPT)
    g.refused(L.slampp_hip_solve_again_device_async(h, None), ERR_INVALID, "solve_again" + NO_KEPT)
    g.refused(L.slampp_hip_solve_again(h, g.hr), ERR_INVALID, "solve_again: no valid factorization")
    g.refused(L.slampp_hip_refine(h, g.hv, g.hr, g.hx, 2, None), ERR_INVALID, "refine" + NO_KEPT)
    g.refused(L.slampp_hip_refine(h, None, None, None, 0, None), ERR_INVALID, "refine" + NO_KEPT)
    g.refused(L.slampp_hip_refine_device_async(h, g.dv, g.dr, g.dx, 2, None), ERR_INVALID, "refine" + NO_KEPT)
    g.ok(g.factor_solve())                                             # (without schur_keep: a factor the handle cannot solve again from)
    g.refused(g.again(), ERR_INVALID, "solve_again" + NO_KEPT)
    g.refused(L.slampp_hip_solve_again(h, g.hr), ERR_UNSUPPORTED, "solve_again: only the sparse path keeps its factor")
    g.refused(L.slampp_hip_solve_again(h, None), ERR_UNSUPPORTED, "solve_again: only the sparse path keeps its factor")
    # an all-reduce callback: the handle is one rank's landmark shard
    g.ok(L.slampp_hip_schur_marginals_pattern(h, g.hv, g.ho))         # (something to reuse and to solve again from)
    g.ok(g.again())
    g.ok(L.slampp_hip_solve_again(h, g.hr))
    g.s.set_allreduce(lambda p, n_doubles, stream: 0)
    for fn, vals, out in ((L.slampp_hip_schur_marginals_pattern, g.hv, g.ho), (L.slampp_hip_schur_marginals_pattern_device_async, g.dv, g.do)):
        g.refused(fn(h, vals, out), ERR_UNSUPPORTED, "schur_marginals_pattern" + ALLREDUCE)
        g.refused(fn(h, None, None), ERR_UNSUPPORTED, "schur_marginals_pattern" + ALLREDUCE)
    for fn, vals, out in ((L.slampp_hip_schur_marginal_columns, g.hv, g.ho), (L.slampp_hip_schur_marginal_columns_device_async, g.dv, g.do)):
        g.refused(fn(h, vals, 2, g.hc, out), ERR_UNSUPPORTED, "schur_marginal_columns" + ALLREDUCE)
        g.refused(fn(h, None, 0, None, None), ERR_UNSUPPORTED, "schur_marginal_columns" + ALLREDUCE)
    g.refused(g.again(), ERR_UNSUPPORTED, "solve_again" + SHARDS)
    g.refused(L.slampp_hip_solve_again(h, g.hr), ERR_UNSUPPORTED, "solve_again" + SHARDS)
    g.refused(L.slampp_hip_refine(h, g.hv, g.hr, g.hx, 2, None), ERR_UNSUPPORTED, "refine" + SHARDS)
    g.refused(L.slampp_hip_refine_device_async(h, g.dv, g.dr, g.dx, 2, None), ERR_UNSUPPORTED, "refine" + SHARDS)
    g.s.set_allreduce(None)
    g.ok(g.pattern_null())                                             # (the refusals changed nothing)
    g.ok(g.again())
    g.ok(g.sync())


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="handles over several devices need two of them")
def test_refusals_over_several_devices(chain, ba):
    over = ": not for a handle over several devices"
    g = Handle(CLinearSolver_HIP(devices=[0, 1]), chain)                # (a pose graph: the handle stays a plain solver on the first device)
    L, h = g.lib, g.h
    g.refused(L.slampp_hip_marginals_pattern(h, g.hv, g.ho), ERR_UNSUPPORTED, "marginals_pattern" + over)
    g.refused(L.slampp_hip_marginals_pattern_device_async(h, g.dv, g.do), ERR_UNSUPPORTED, "marginals_pattern" + over)
    g.refused(L.slampp_hip_marginal_columns(h, g.hv, 2, g.hc, g.ho), ERR_UNSUPPORTED, "marginal_columns" + over)
    g.refused(L.slampp_hip_marginal_columns_device_async(h, g.dv, 2, g.hc, g.do), ERR_UNSUPPORTED, "marginal_columns" + over)
    g = Handle(CLinearSolver_Schur_HIP(devices=[0, 1]), ba)
    L, h = g.lib, g.h
    g.refused(L.slampp_hip_schur_marginals_pattern(h, g.hv, g.ho), ERR_UNSUPPORTED, "schur_marginals_pattern" + over)
    g.refused(L.slampp_hip_schur_marginals_pattern_device_async(h, g.dv, g.do), ERR_UNSUPPORTED, "schur_marginals_pattern" + over)
    g.refused(L.slampp_hip_schur_marginal_columns(h, g.hv, 2, g.hc, g.ho), ERR_UNSUPPORTED, "schur_marginal_columns" + over)
    g.refused(L.slampp_hip_schur_marginal_columns_device_async(h, g.dv, 2, g.hc, g.do), ERR_UNSUPPORTED, "schur_marginal_columns" + over)
    g.refused(L.slampp_hip_schur_marginals_device_async(h, g.dv, g.do, None), ERR_INVALID,
              "schur_marginals_device: this handle solves with landmark shards on several devices: host entry points only")
    g.refused(L.slampp_hip_solve_marginal_poses_device_async(h, g.dv, g.dr), ERR_INVALID,
              "solve_marginal_poses_device: this handle solves with landmark shards on several devices: host entry points only")
    g.refused(g.again(), ERR_UNSUPPORTED, "solve_again" + SHARDS)
    g.refused(L.slampp_hip_multiply(h, g.hv, g.hx, g.hy, 1.0, 0.0), ERR_UNSUPPORTED,
              "multiply: this handle solves with landmark shards on several devices")
    g.refused(L.slampp_hip_refine(h, g.hv, g.hr, g.hx, 2, None), ERR_UNSUPPORTED,
              "refine: this handle solves with landmark shards on several devices")


# ---- the factor state ----

def sparse_state(g, b_factor):
    """solve_again and marginal_columns(values = NULL) are accepted exactly while the sparse handle holds a factor."""
    if b_factor:
        g.ok(g.again())
        g.ok(g.cols_null())
    else:
        g.refused(g.again(), ERR_INVALID, "solve_again: no valid factorization")
        g.refused(g.cols_null(), ERR_INVALID, COLS_NO_REUSE)


def test_sparse_factor_state(chain):
    g = Handle(CLinearSolver_HIP(dense_top_nb=0), chain)
    L, h = g.lib, g.h
    assert g.s.plan()["dense_dim"] == 0
    sparse_state(g, False)                                             # analyzed, nothing factored
    g.ok(g.factor_solve())
    sparse_state(g, True)
    g.ok(g.set_structure())
    g.refused(g.again(), ERR_INVALID, "solve_again: no valid factorization (analyze was not called)")
    g.refused(g.cols_null(), ERR_INVALID, "marginal_columns: analyze was not called")
    g.ok(L.slampp_hip_analyze(h, 0, 0))
    sparse_state(g, False)                                             # (the analysis brings no factor back)
    g.ok(L.slampp_hip_factorize(h, g.hv, g.ho))                        # no dense top: the factor can be solved from
    sparse_state(g, True)
    g.ok(L.slampp_hip_analyze(h, 0, 0))
    sparse_state(g, False)
    g.ok(L.slampp_hip_marginals(h, g.hv, g.ho))
    sparse_state(g, True)
    g.ok(L.slampp_hip_analyze(h, 0, 0))
    g.ok(L.slampp_hip_marginals_pattern(h, g.hv, g.ho))
    sparse_state(g, True)
    g.ok(L.slampp_hip_analyze(h, 0, 0))
    g.ok(L.slampp_hip_marginal_columns(h, g.hv, 2, g.hc, g.ho))
    sparse_state(g, True)
    # batches: one member's factor is the handle's; two members in one pass of launches leave the handle's own factor alone
    n, nv = chain.n_scalars, chain.values.shape[0]
    t_vals2, t_rhs2 = torch.cat([g.t_vals, g.t_vals]), dev(2 * n)
    status = (C.c_int * 2)()
    g.ok(L.slampp_hip_analyze(h, 0, 0))
    sparse_state(g, False)
    g.ok(L.slampp_hip_factor_solve_batch_device_async(h, 2, t_vals2.data_ptr(), nv, t_rhs2.data_ptr(), n))
    g.ok(L.slampp_hip_sync_batch(h, status, 2))
    assert list(status) == [OK, OK]
    sparse_state(g, False)
    g.ok(L.slampp_hip_factor_solve_batch_device_async(h, 1, t_vals2.data_ptr(), nv, t_rhs2.data_ptr(), n))
    sparse_state(g, True)
    g.ok(L.slampp_hip_sync_batch(h, status, 1))
    assert status[0] == OK
    sparse_state(g, True)
    g.ok(L.slampp_hip_factor_solve_batch_device_async(h, 2, t_vals2.data_ptr(), nv, t_rhs2.data_ptr(), n))
    g.ok(L.slampp_hip_sync_batch(h, status, 2))
    sparse_state(g, True)


def test_sparse_factor_state_with_dense_top(chain):
    g = Handle(CLinearSolver_HIP(dense_top_nb=2, dense_top_min_dim=0), chain)
    L, h = g.lib, g.h
    assert g.s.plan()["dense_dim"] > 0
    sparse_state(g, False)
    g.ok(g.factor_solve())
    sparse_state(g, True)
    g.ok(L.slampp_hip_factorize(h, g.hv, g.ho))                        # the substitutions' vectors were not brought along
    sparse_state(g, False)
    g.ok(L.slampp_hip_marginal_columns(h, g.hv, 2, g.hc, g.ho))
    sparse_state(g, True)
    # two members go through the handle's own factor arrays and its dense top one after the other: declared gone
    n, nv = chain.n_scalars, chain.values.shape[0]
    t_vals2, t_rhs2 = torch.cat([g.t_vals, g.t_vals]), dev(2 * n)
    status = (C.c_int * 2)()
    g.ok(L.slampp_hip_factor_solve_batch_device_async(h, 2, t_vals2.data_ptr(), nv, t_rhs2.data_ptr(), n))
    sparse_state(g, False)
    g.ok(L.slampp_hip_sync_batch(h, status, 2))
    assert list(status) == [OK, OK]
    sparse_state(g, False)
    g.ok(L.slampp_hip_factor_solve_batch_device_async(h, 1, t_vals2.data_ptr(), nv, t_rhs2.data_ptr(), n))
    g.ok(L.slampp_hip_sync_batch(h, status, 1))
    sparse_state(g, True)


def test_not_positive_definite_drops_the_factor():
    from golden_util import load_golden
    bad, _ = load_golden("indefinite_n40")
    off = bad.block_value_offsets()
    k = int(bad.bcol_ptr[bad.n_bcols // 2 + 1] - 1)                    # (synth.indefinite: 50 taken off this diagonal block)
    good_vals = bad.values.copy()
    good_vals[off[k]:off[k + 1]] += (50.0 * np.eye(6)).ravel()
    g = Handle(CLinearSolver_HIP(), bad)
    L, h = g.lib, g.h
    g.ok(g.factor_solve(good_vals))
    sparse_state(g, True)
    rc = g.factor_solve()
    assert (rc, g.s._error()) == (NOT_POSDEF, "matrix is not positive definite")
    sparse_state(g, False)
    g.ok(g.factor_solve(good_vals))
    sparse_state(g, True)
    g.ok(L.slampp_hip_factor_solve_device_async(h, g.dv, g.dr))        # enqueued: the answer comes with the sync
    assert (g.sync(), g.s._error()) == (NOT_POSDEF, "matrix is not positive definite")
    sparse_state(g, False)
    g.ok(g.sync())                                                     # (answered for)
    sparse_state(g, False)
    # a batch of one whose member fails: the factor the handle kept is dropped at sync_batch
    g.ok(g.factor_solve(good_vals))
    status = (C.c_int * 1)()
    g.ok(L.slampp_hip_factor_solve_batch_device_async(h, 1, g.dv, int(bad.values.shape[0]), g.dr, int(bad.n_scalars)))
    g.ok(L.slampp_hip_sync_batch(h, status, 1))
    assert status[0] == NOT_POSDEF
    sparse_state(g, False)


def schur_state(g, b_again, b_reuse):
    """Schur mode: solve_again takes what a keeping solve or a covariance call left; values = NULL only the latter."""
    if b_again:
        g.ok(g.again())
    else:
        g.refused(g.again(), ERR_INVALID, "solve_again" + NO_KEPT)
    if b_reuse:
        g.ok(g.pattern_null())
    else:
        g.refused(g.pattern_null(), ERR_INVALID, "schur_marginals_pattern" + NO_REUSE)


@pytest.mark.parametrize("keep", [0, 1])
def test_schur_factor_state(ba, keep):
    g = Handle(CLinearSolver_Schur_HIP(schur_keep=keep), ba)
    L, h = g.lib, g.h
    b_keep = bool(keep)
    cut = int(ba.n_matrix_cut)
    schur_state(g, False, False)                                       # analyzed, nothing factored
    g.ok(g.factor_solve())
    schur_state(g, b_keep, False)
    g.ok(L.slampp_hip_schur_marginals_pattern(h, g.hv, g.ho))
    schur_state(g, True, True)
    schur_state(g, True, True)                                         # (values = NULL itself counts nothing up)
    g.ok(g.factor_solve())
    schur_state(g, b_keep, False)
    g.ok(L.slampp_hip_schur_marginal_columns(h, g.hv, 2, g.hc, g.ho))
    schur_state(g, True, True)
    g.ok(L.slampp_hip_schur_marginal_columns(h, None, 2, g.hc, g.ho))
    schur_state(g, True, True)
    g.ok(L.slampp_hip_schur_marginals(h, g.hv, g.ho, None))            # C^-1 and W recomputed: nothing kept matches them
    schur_state(g, False, False)
    g.ok(L.slampp_hip_schur_marginals_pattern(h, g.hv, g.ho))
    g.ok(L.slampp_hip_solve_marginal_poses(h, g.hv, _ptr(g.rhs.copy())))
    schur_state(g, False, False)
    g.ok(L.slampp_hip_schur_marginals_pattern(h, g.hv, g.ho))
    g.ok(g.set_structure())
    g.refused(g.again(), ERR_INVALID, "solve_again: no valid factorization (analyze was not called)")
    g.refused(g.pattern_null(), ERR_INVALID, "schur_marginals_pattern: analyze was not called")
    g.ok(L.slampp_hip_analyze(h, 1, cut))
    schur_state(g, False, False)
    g.ok(g.factor_solve())
    schur_state(g, b_keep, False)
    g.ok(g.sync())


# ---- the grouping of block columns ----

def groups_of(dims):
    """The passes of slampp_hip_marginal_columns: whole block columns, at most COV_K_PASS scalar columns each."""
    groups, k = [[]], 0
    for d in dims:
        if groups[-1] and k + d > COV_K_PASS:
            groups.append([])
            k = 0
        groups[-1].append(int(d))
        k += int(d)
    return groups


def check_grouping(solver, lam, cols):
    dims = np.diff(lam.cumsum)[cols]
    groups = groups_of(dims)
    assert len(groups) >= 3                                            # the width crosses COV_K_PASS at least twice
    assert any(a[-1] != b[0] for a, b in zip(groups, groups[1:]))      # a boundary between two blocks of different width
    X = solver.Marginal_Columns(lam, cols)
    assert X.shape == (lam.n_scalars, int(dims.sum()))
    single = [solver.Marginal_Columns(lam, [c], reuse_factor=True) for c in cols]
    assert np.array_equal(X, np.concatenate(single, axis=1))
    assert np.array_equal(X, solver.Marginal_Columns(lam, cols, reuse_factor=True))


def test_grouping_sparse():
    from test_covariance_blocks_gpu import mixed_system
    lam, _ = mixed_system(700)
    rng = np.random.default_rng(3)
    cols = rng.permutation(lam.n_bcols)[:30].tolist()
    check_grouping(CLinearSolver_HIP(dense_top_nb=0), lam, cols)


def test_grouping_schur(ba):
    nc = int(ba.n_matrix_cut)
    cols = list(range(7)) + [nc] + [7] + list(range(nc + 1, nc + 22))    # 42 + 3 | 6 + ...: a pass ends between a landmark and a camera
    check_grouping(CLinearSolver_Schur_HIP(), ba, cols)
