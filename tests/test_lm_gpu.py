"""The Levenberg-Marquardt loop decided on the device (csrc/lm.hip, csrc/capi_lm.hip) on the GPU: the building blocks one by
one, then slampp_hip_lm_begin_device_async / slampp_hip_lm_iterate_device_async on the three fixtures of tests/golden/linearize/
(40 SE(2) poses, 40 SE(3) poses, 6 cameras x 40 points) against the model of tests/lm_model.py.

Decisions, status and counters are compared exactly.  The figures of a loop (alpha, chi^2, rho, |dx|, the final state) are
compared to lm_model.tolerance(kind): per fixture and quantity, 100 times what solving by Cholesky or by LU moves that quantity in
the model (tests/test_lm_model_host.py prints it; the figure is measured again wherever the test runs, and moves by a factor of
two or three with the BLAS underneath numpy), and not below the project's 1e-10.  Measured: alpha 2.2e-11 (SE(2)), 1.6e-10
(SE(3)), 0 (BA); chi^2 below 1.6e-14; the state below 7e-16; |dx| 8.2e-9, 1.6e-10, 2.5e-10; rho 3.3e-9 (SE(3)), 1.1e-5 (BA) and
7.7e-2 on SE(2), whose last rounds move chi^2 in its 12th digit and form rho from cancelled figures -- so the tolerances are
alpha 2.2e-9 / 1.6e-8 / 1e-10, chi^2 and state 1e-10, |dx| 8.2e-7 / 1.6e-8 / 2.5e-8, rho 3.3e-7 (SE(3)), 1.1e-3 (BA) and none
worth the name on SE(2), where the exact comparison of the accept flags stands in."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import linearize_model as M
import lm_model as L
from slam_plus_plus_amd import synth
from slam_plus_plus_amd import hip_solver as H
from slam_plus_plus_amd.hip_solver import (CLambdaAssembly_HIP, CLevenbergMarquardt_HIP, CLinearSolver_HIP, CLinearSolver_Schur_HIP,
                                           EDGE_P2C_XYZ, EDGE_SE2, EDGE_SE3, ERR_INVALID, ERR_UNSUPPORTED, VERTEX_EUCLIDEAN, VERTEX_SE2,
                                           VERTEX_SE3)

pytestmark = pytest.mark.gpu
TOL = 1e-10
EDGE_TYPE = {"se2": EDGE_SE2, "se3": EDGE_SE3, "ba": EDGE_P2C_XYZ}
SENTINEL = -7.25e300
N_GUARD = 16

# the model's constants are the header's
assert [getattr(H, "LM_" + n) for n in ("ALPHA", "NU", "LAST_ERROR", "ERROR", "DX_DX", "DX_ETA", "RHO", "ACCEPTED", "STATUS", "N_ROUNDS",
                                        "N_ACCEPTED", "N_REJECTED", "ROUNDS_LEFT", "EXTRA_LEFT", "MIN_DX_NORM", "N_RECORDS", "SCALARS")] == list(range(17))
assert (H.LM_TRACE_RECORD, H.LM_SCALARS) == (L.RECORD, L.SCALARS)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def guarded(n):
    """n doubles followed by sentinels."""
    return torch.full((n + N_GUARD,), SENTINEL, dtype=torch.float64, device="cuda")


def guard_intact(t, n):
    return bool((t[n:] == SENTINEL).all())


def col_major(J):
    """[E, rd, d] row-major matrices -> the C ABI's column-major blocks."""
    return np.ascontiguousarray(np.transpose(J, (0, 2, 1)))


def vertex_ranges(kind, fx):
    n = len(fx["cumsum"]) - 1
    if kind == "ba":
        return [(VERTEX_SE3, 0, int(fx["n_cams"])), (VERTEX_EUCLIDEAN, int(fx["n_cams"]), n)]
    return [({"se2": VERTEX_SE2, "se3": VERTEX_SE3}[kind], 0, n)]


class Graph:
    """A fixture on the device: the solver, Lambda's structure and an assembly handle over the edge list given (the
    fixture's, n_tile times over, cut to n_edges)."""

    def __init__(self, kind, n_edges=None, n_tile=1, solver_class=None, first_edge=0):
        self.kind, self.fx = kind, M.load_fixture(kind)
        fx = self.fx
        self.d0, self.d1, self.rd = M.EDGE_SHAPES[kind]
        self.dims = np.diff(fx["cumsum"])
        self.lam = synth.structure_from_edges(self.dims, fx["v0"], fx["v1"])
        if kind == "ba":
            self.lam.n_matrix_cut = int(fx["n_cams"])
        self.solver = (solver_class or (CLinearSolver_Schur_HIP if kind == "ba" else CLinearSolver_HIP))()
        v0, v1 = np.tile(fx["v0"], n_tile)[first_edge:], np.tile(fx["v1"], n_tile)[first_edge:]
        self.n_edges = len(v0) if n_edges is None else n_edges
        self.cut = slice(first_edge, first_edge + self.n_edges)
        self.n_tile = n_tile
        self.asm = CLambdaAssembly_HIP(self.solver, self.lam, v0[:self.n_edges], v1[:self.n_edges], self.rd)
        self.state = dev(fx["state"])
        self.z = dev(np.tile(fx["z"], (n_tile, 1))[self.cut])
        self.params = None if fx["params"] is None else dev(fx["params"])
        self.sigma_inv_host = np.tile(fx["sigma_inv"], (n_tile, 1, 1))[self.cut]
        self.sigma_inv = dev(col_major(self.sigma_inv_host))
        self.n_scalars, self.n_bcols = int(fx["cumsum"][-1]), len(self.dims)

    def model_jacobians(self):
        """(J0, J1) of the model for this edge list, [E, rd, d] row-major."""
        _, _, J0, J1 = M.fixture_model(self.kind)
        return np.tile(J0, (self.n_tile, 1, 1))[self.cut], np.tile(J1, (self.n_tile, 1, 1))[self.cut]

    def set_ptrs(self, J0, J1, weight=None):
        return (self.asm, J0, J1, self.sigma_inv, weight)


def initial_damping(sets, tau, solver):
    """slampp_hip_lm_initial_damping_device_async over (assembly, J0, J1, sigma_inv, weight) tuples of device tensors."""
    arr = (H.EdgeSetPtrs * len(sets))()
    for i, (asm, J0, J1, sigma, weight) in enumerate(sets):
        arr[i].p_assembly, arr[i].p_J0_dev, arr[i].p_J1_dev, arr[i].p_sigma_inv_dev = asm._a, J0.data_ptr(), J1.data_ptr(), sigma.data_ptr()
        arr[i].p_weight_dev = None if weight is None else weight.data_ptr()
    out = torch.full((1 + N_GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    solver._check(solver._lib.slampp_hip_lm_initial_damping_device_async(arr, len(sets), float(tau), out.data_ptr()))
    assert solver.sync() and guard_intact(out, 1)
    return float(out[0])


# ---- the initial damping ----

@pytest.mark.parametrize("kind", M.KINDS)
def test_initial_damping_on_the_fixtures(kind):
    g = Graph(kind)
    J0, J1 = g.model_jacobians()
    ref = L.TAU * L.initial_damping(J0, J1, g.sigma_inv_host)
    got = initial_damping([g.set_ptrs(dev(col_major(J0)), dev(col_major(J1)))], L.TAU, g.solver)
    assert ref > 0 and abs(got - ref) < TOL * ref
    w = np.random.default_rng(4).uniform(0.2, 1.0, g.n_edges)
    ref_w = L.initial_damping(J0, J1, g.sigma_inv_host, w)
    got_w = initial_damping([g.set_ptrs(dev(col_major(J0)), dev(col_major(J1)), dev(w))], 1.0, g.solver)
    assert abs(got_w - ref_w) < TOL * ref_w and got_w < got / L.TAU


@pytest.mark.parametrize("n_edges", [1, 63, 64, 65, 165, 715])
def test_initial_damping_edge_counts(n_edges):
    """The SE(3) edge list tiled (3 x 55 = 165; 13 x 55 = 715 edges take three workgroups of 256 and the second pass).  The
    last edge's Jacobians are multiplied by 16, so that the maximum sits in the last lane that has an edge."""
    g = Graph("se3", n_edges, n_tile=13)
    J0, J1 = (J.copy() for J in g.model_jacobians())
    J0[-1] *= 16
    J1[-1] *= 16
    ref = L.initial_damping(J0, J1, g.sigma_inv_host)
    last = L.initial_damping(J0[-1:], J1[-1:], g.sigma_inv_host[-1:])
    d0, d1 = guarded(J0.size), guarded(J1.size)
    d0[:J0.size], d1[:J1.size] = dev(col_major(J0)).ravel(), dev(col_major(J1)).ravel()
    got = initial_damping([g.set_ptrs(d0, d1)], 1.0, g.solver)
    assert ref == last and abs(got - ref) < TOL * ref
    assert initial_damping([g.set_ptrs(d0, d1)], 1.0, g.solver) == got


def test_initial_damping_two_sets_against_their_union():
    whole, a, b = Graph("se3"), Graph("se3", 20), Graph("se3", 35, first_edge=20)
    J0, J1 = whole.model_jacobians()
    up = lambda J, cut: dev(col_major(J[cut]))
    union = initial_damping([whole.set_ptrs(up(J0, slice(None)), up(J1, slice(None)))], L.TAU, whole.solver)
    # the two assemblies of one call belong to one solver
    b_asm = CLambdaAssembly_HIP(a.solver, a.lam, a.fx["v0"][20:], a.fx["v1"][20:], 6)
    sets = [a.set_ptrs(up(J0, slice(0, 20)), up(J1, slice(0, 20))), (b_asm, up(J0, slice(20, 55)), up(J1, slice(20, 55)), b.sigma_inv, None)]
    both = initial_damping(sets, L.TAU, a.solver)
    each = [initial_damping([s], L.TAU, a.solver) for s in sets]
    assert both == union == max(each) and min(each) > 0


# ---- errors only ----

@pytest.mark.parametrize("kind,n_tile", [("se2", 1), ("se3", 1), ("ba", 1), ("se3", 3)])
def test_errors_only_has_the_bits_of_linearize(kind, n_tile):
    g = Graph(kind, n_tile=n_tile)
    n = g.n_edges
    J0, J1, err, only = guarded(n * g.rd * g.d0), guarded(n * g.rd * g.d1), guarded(n * g.rd), guarded(n * g.rd)
    params = 0 if g.params is None else g.params.data_ptr()
    torch.cuda.synchronize()
    g.asm.Linearize_device(EDGE_TYPE[kind], g.state.data_ptr(), g.z.data_ptr(), J0.data_ptr(), J1.data_ptr(), err.data_ptr(), params)
    g.solver._check(g.solver._lib.slampp_hip_edge_errors_device_async(g.asm._a, EDGE_TYPE[kind], g.state.data_ptr(), g.z.data_ptr(),
                                                                   params or None, only.data_ptr()))
    assert g.solver.sync()
    assert torch.equal(only, err) and guard_intact(only, n * g.rd) and not bool((only[:n * g.rd] == SENTINEL).any())


# ---- damping from a device scalar ----

@pytest.mark.parametrize("kind", ["se3", "ba"])
def test_scalar_damping_has_the_bits_of_apply_damping(kind):
    g = Graph(kind)
    nv, n = g.lam.values.shape[0], g.n_bcols
    values = dev(np.random.default_rng(1).normal(size=nv))
    alpha = 0.3718281828
    alpha_dev = dev([alpha])
    for scale, (first, last) in ((1.0, (0, n)), (-1.0, (0, n)), (1.0, (3, n - 2)), (1.0, (5, 5))):
        a, b = guarded(nv), guarded(nv)
        a[:nv], b[:nv] = values, values
        torch.cuda.synchronize()
        g.solver.apply_damping_device_async(a.data_ptr(), scale * alpha, first, last)
        g.solver._check(g.solver._lib.slampp_hip_apply_damping_scalar_device_async(g.solver._h, b.data_ptr(), alpha_dev.data_ptr(), scale,
                                                                                first, last))
        assert g.solver.sync()
        assert torch.equal(a, b) and guard_intact(b, nv) and (first == last) == torch.equal(b[:nv], values)


# ---- the gain ratio's two sums ----

@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 5000])
def test_gain(n):
    """A workgroup of the first pass spans 1024 entries (the partition of slampp_hip_dot_device_async): 1025 and 5000 take more
    than one partial result.  Each sum within n 2^-52 sum |a_i b_i| of the exactly rounded sum."""
    dims = np.array([8] * (n // 8) + ([n % 8] if n % 8 else []))
    lam = synth.structure_from_edges(dims, np.zeros(0, np.int64), np.zeros(0, np.int64))
    solver = CLinearSolver_HIP()
    solver._set_structure(lam)
    rng = np.random.default_rng(n)
    dx, eta = rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, n), rng.normal(size=n)
    d_dx, d_eta = dev(dx), dev(eta)
    lm = torch.full((2, L.SCALARS + N_GUARD), SENTINEL, dtype=torch.float64, device="cuda")
    lm[:, L.STATUS] = 0
    torch.cuda.synchronize()
    for k in range(2):
        solver._check(solver._lib.slampp_hip_lm_gain_device_async(solver._h, d_dx.data_ptr(), d_eta.data_ptr(), lm[k].data_ptr()))
    assert solver.sync()
    got = lm.cpu().numpy()
    for col, b in ((L.DX_DX, dx), (L.DX_ETA, eta)):
        exact, bound = math.fsum(dx * b), n * 2.0 ** -52 * math.fsum(np.abs(dx * b))
        print(f"gain n = {n}: error {abs(got[0, col] - exact):.3g}, bound {bound:.3g}")
        assert abs(got[0, col] - exact) <= bound
    assert np.array_equal(got[0], got[1])
    untouched = np.ones(L.SCALARS + N_GUARD, bool)
    untouched[[L.DX_DX, L.DX_ETA, L.STATUS]] = False
    assert np.all(got[0][untouched] == SENTINEL)
    # a block whose status is set is left alone
    lm[0, L.STATUS] = 1
    lm[0, L.DX_DX] = 5.0
    torch.cuda.synchronize()
    solver._check(solver._lib.slampp_hip_lm_gain_device_async(solver._h, d_eta.data_ptr(), d_eta.data_ptr(), lm[0].data_ptr()))
    assert solver.sync() and float(lm[0, L.DX_DX]) == 5.0


# ---- the decision ----

def crafted_blocks():
    """(name, scalars, chi^2 parts, trace capacity): LAST_ERROR 10, ALPHA 2, dx^T dx = 1, dx^T eta = 2 -- the denominator is 4."""
    def block(**kw):
        s = L.begin(2.0, 10.0, 1e-6, 5, 2)
        s[L.DX_DX], s[L.DX_ETA] = 1.0, 2.0
        for k, v in kw.items():
            s[getattr(L, k)] = v
        return s
    cases = [("rho 0.9", block(), [10.0 - 4 * 0.9], 1), ("rho 0.5", block(), [8.0], 1),
             ("rho 1e-3: the cap, not 1/3", block(), [10.0 - 4e-3], 1), ("rho 1.5: 1/3", block(), [4.0], 1),
             ("two parts", block(), [3.0, 3.4], 1), ("rho 0", block(), [10.0], 1), ("rho < 0", block(), [11.0], 1),
             ("NaN chi2", block(), [float("nan")], 1), ("rho < 0 from nu 64", block(NU=64.0, N_REJECTED=5.0), [10.5], 1),
             ("converged", block(DX_DX=1e-14), [9.0], 1), ("converged at equality", block(DX_DX=2.0 ** -40, MIN_DX_NORM=2.0 ** -20), [9.0], 1),
             ("last round, accepted", block(ROUNDS_LEFT=1), [8.0], 1), ("last round, rejected, no extra", block(ROUNDS_LEFT=1, EXTRA_LEFT=0), [11.0], 1),
             ("last round, rejected, one extra", block(ROUNDS_LEFT=1, EXTRA_LEFT=1), [11.0], 1),
             ("status already set", block(STATUS=3.0, ACCEPTED=1.0, ROUNDS_LEFT=0), [8.0], 1),
             ("converged already", block(STATUS=1.0), [8.0], 1), ("no room in the trace", block(N_RECORDS=1.0), [8.0], 1),
             ("no trace", block(), [8.0], 0)]
    return cases


def test_decide_against_the_rule():
    g = Graph("se3")                                   # (an analyzed handle: the decision reads its flag)
    g.solver.SymbolicDecomposition_Blocky(g.lam)
    cases = crafted_blocks()
    k = len(cases)
    lm = torch.full((k, L.SCALARS + N_GUARD), SENTINEL, dtype=torch.float64, device="cuda")
    parts = torch.zeros((k, 2), dtype=torch.float64, device="cuda")
    trace = torch.full((k, L.RECORD + N_GUARD), SENTINEL, dtype=torch.float64, device="cuda")
    for i, (_, s, chi, _) in enumerate(cases):
        lm[i, :L.SCALARS] = dev(s)
        parts[i, :len(chi)] = dev(chi)
    torch.cuda.synchronize()
    for i, (_, s, chi, capacity) in enumerate(cases):
        g.solver._check(g.solver._lib.slampp_hip_lm_decide_device_async(g.solver._h, lm[i].data_ptr(), parts[i].data_ptr(), len(chi),
                                                                     trace[i].data_ptr() if capacity else None, capacity))
    assert g.solver.sync()
    lm, trace = lm.cpu().numpy(), trace.cpu().numpy()
    for i, (name, s, chi, capacity) in enumerate(cases):
        want, want_trace = s.copy(), np.full((1, L.RECORD), SENTINEL)
        L.decide(want, False, chi, want_trace if capacity else None)
        got = lm[i, :L.SCALARS]
        assert np.all(lm[i, L.SCALARS:] == SENTINEL) and np.all(trace[i, L.RECORD:] == SENTINEL), name
        exact = [c for c in range(L.SCALARS) if c != L.ALPHA]
        assert np.array_equal(got[exact], want[exact], equal_nan=True), (name, got, want)
        assert abs(got[L.ALPHA] - want[L.ALPHA]) <= 4 * np.spacing(want[L.ALPHA]), (name, got[L.ALPHA], want[L.ALPHA])
        cols = [c for c in range(L.RECORD) if c != L.T_ALPHA]
        assert np.array_equal(trace[i, :L.RECORD][cols], want_trace[0][cols], equal_nan=True), (name, trace[i], want_trace)
        assert trace[i, L.T_ALPHA] == want_trace[0, L.T_ALPHA], name
    by_name = {name: lm[i] for i, (name, *_rest) in enumerate(cases)}
    assert by_name["rho 1e-3: the cap, not 1/3"][L.ALPHA] > 3.9 and by_name["rho 1.5: 1/3"][L.ALPHA] == 2 / 3.0
    assert by_name["NaN chi2"][L.ACCEPTED] == 0 and by_name["converged at equality"][L.STATUS] == L.CONVERGED
    assert by_name["last round, rejected, one extra"][L.STATUS] == L.RUNNING and by_name["last round, rejected, no extra"][L.STATUS] == L.BUDGET


# ---- the commit ----

@pytest.mark.parametrize("n", [1, 2, 3, 255, 256, 257, 1029])
def test_commit(n):
    dims = np.array([8] * (n // 8) + ([n % 8] if n % 8 else []))
    lam = synth.structure_from_edges(dims, np.zeros(0, np.int64), np.zeros(0, np.int64))
    solver = CLinearSolver_HIP()
    solver._set_structure(lam)
    lm = torch.zeros((2, L.SCALARS), dtype=torch.float64, device="cuda")
    lm[1, L.ACCEPTED] = 1
    for off_state, off_trial in ((0, 0), (1, 1), (0, 1), (1, 0)):        # pointers offset by one double: 8-byte alignment only
        for accepted in (0, 1):
            state, trial = guarded(n + 2), guarded(n + 2)
            state[off_state:off_state + n] = torch.arange(n, dtype=torch.float64, device="cuda")
            trial[off_trial:off_trial + n] = -1 - torch.arange(n, dtype=torch.float64, device="cuda")
            before = state.clone()
            torch.cuda.synchronize()
            solver._check(solver._lib.slampp_hip_lm_commit_device_async(solver._h, lm[accepted].data_ptr(), state.data_ptr() + 8 * off_state,
                                                                     trial.data_ptr() + 8 * off_trial))
            assert solver.sync()
            if accepted:
                assert torch.equal(state[off_state:off_state + n], trial[off_trial:off_trial + n])
                assert torch.equal(state[:off_state], before[:off_state]) and torch.equal(state[off_state + n:], before[off_state + n:])
            else:
                assert torch.equal(state, before)


# ---- the loop ----

def make_lm(kind, solver_class=None, trace_capacity=64, unary="default"):
    g = Graph(kind, solver_class=solver_class)
    sets = [dict(assembly=g.asm, edge_type=EDGE_TYPE[kind], measurement=g.z, sigma_inv=g.sigma_inv, params=g.params)]
    if isinstance(unary, str):
        unary = L.unary_of(kind, g.fx)
    elif unary is not None:                             # (the factor column-major, as the assembly reads it)
        unary = (unary[0], np.ascontiguousarray(np.asarray(unary[1]).T), unary[2])
    lm = CLevenbergMarquardt_HIP(g.solver, g.lam, sets, vertex_ranges(kind, g.fx), g.fx["state"], unary, trace_capacity)
    lm.graph = g
    return lm


_runs = {}


def device_run(kind, solver_class=None):
    """The loop of lm_model.LOOPS on the device, once per process: every round enqueued, one wait."""
    key = (kind, solver_class)
    if key not in _runs:
        n_rounds, f_min_dx_norm = L.LOOPS[kind]
        lm = make_lm(kind, solver_class)
        lm.Begin(0.0, L.TAU, f_min_dx_norm)
        lm.Iterate(n_rounds)
        ok, scalars, trace = lm.Sync()
        _runs[key] = dict(ok=ok, scalars=scalars, trace=trace, state=lm.state.cpu().numpy(), lm=lm)
    return _runs[key]


def compare_with_model(kind, run, model):
    tol = L.tolerance(kind)
    t, tm, s, sm = run["trace"], model["trace"], run["scalars"], model["scalars"]
    assert run["ok"] and t.shape == tm.shape
    for col in (L.T_ACCEPTED, L.T_STATUS, L.T_NU):
        assert np.array_equal(t[:, col], tm[:, col]), (col, t[:, col], tm[:, col])
    ints = [L.NU, L.ACCEPTED, L.STATUS, L.N_ROUNDS, L.N_ACCEPTED, L.N_REJECTED, L.ROUNDS_LEFT, L.EXTRA_LEFT, L.MIN_DX_NORM, L.N_RECORDS]
    assert np.array_equal(s[ints], sm[ints]), (s, sm)
    k = L.compared_rounds(model)
    for q, col in (("alpha", L.T_ALPHA), ("chi2", L.T_ERROR), ("chi2", L.T_LAST_ERROR), ("rho", L.T_RHO), ("dx_norm", L.T_DX_NORM)):
        gap = np.abs(t[:k, col] - tm[:k, col]) / np.abs(tm[:k, col])
        print(f"lm {kind}: {q} (trace column {col}) from the model by {gap.max():.3g}, tolerance {tol[q]:.3g}")
        assert np.all(gap <= tol[q]), (q, col, gap)
    assert abs(s[L.LAST_ERROR] - sm[L.LAST_ERROR]) <= tol["chi2"] * sm[L.LAST_ERROR]
    gap = np.abs(run["state"] - model["state"]).max() / np.abs(model["state"]).max()
    print(f"lm {kind}: the final state from the model by {gap:.3g}, tolerance {tol['state']:.3g}")
    assert gap <= tol["state"]


@pytest.mark.parametrize("kind", M.KINDS)
def test_loop_against_the_model(kind):
    """SE(2) and SE(3): 14 rounds; BA (Schur mode) with f_min_dx_norm = 1e-6: 8 rounds enqueued, converged in the fifth."""
    compare_with_model(kind, device_run(kind), L.fixture_run(kind))


def test_ba_loop_on_the_sparse_solver():
    compare_with_model("ba", device_run("ba", CLinearSolver_HIP), L.fixture_run("ba"))


@pytest.mark.parametrize("solver_class", [CLinearSolver_Schur_HIP, CLinearSolver_HIP])
def test_rounds_after_convergence_are_inert(solver_class):
    """BA converges in the fifth of eight rounds: five rounds and a wait, then three more, leave state, scalars and trace
    as the five left them -- and as all eight in one go do."""
    whole = device_run("ba", solver_class)
    lm = make_lm("ba", solver_class)
    lm.Begin(0.0, L.TAU, L.LOOPS["ba"][1])
    lm.Iterate(5)
    ok, scalars, trace = lm.Sync()
    state = lm.state.clone()
    trace_all = lm.trace_dev.clone()
    assert ok and scalars[L.STATUS] == L.CONVERGED and scalars[L.N_ROUNDS] == 5
    lm.Iterate(3)
    ok, scalars_after, trace_after = lm.Sync()
    assert ok and torch.equal(lm.state, state) and torch.equal(lm.trace_dev, trace_all)
    assert np.array_equal(scalars_after, scalars) and np.array_equal(trace_after, trace)
    assert np.array_equal(whole["scalars"], scalars) and np.array_equal(whole["trace"], trace) and np.array_equal(whole["state"], state.cpu().numpy())


def test_one_round_at_a_time_has_the_bits_of_fourteen():
    """Iterate(1) fourteen times with a wait between against Iterate(14); and the state after each rejected round of the SE(3)
    loop is the state before it, bit for bit."""
    whole = device_run("se3")
    lm = make_lm("se3")
    lm.Begin(0.0, L.TAU, 0.0)
    states = [lm.state.clone()]
    for _ in range(14):
        lm.Iterate(1)
        ok, scalars, trace = lm.Sync()
        assert ok
        states.append(lm.state.clone())
    assert np.array_equal(scalars, whole["scalars"]) and np.array_equal(trace, whole["trace"])
    assert np.array_equal(states[-1].cpu().numpy(), whole["state"])
    accepted = trace[:, L.T_ACCEPTED]
    assert list(accepted) == [1, 1, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1]
    for k in range(14):
        assert torch.equal(states[k + 1], states[k]) == (accepted[k] == 0), k


def test_budget_of_extra_iterations():
    """Optimize(3) on the SE(3) fixture: eight solves (five rejected steps are granted an iteration each), status 3."""
    lm = make_lm("se3")
    ok, scalars, trace = lm.Optimize(3, 0.0)
    model = L.run("se3", 13, n_max_iterations=3, n_extra_on_reject=10)
    assert ok and (scalars[L.STATUS], scalars[L.N_ROUNDS], scalars[L.N_ACCEPTED], scalars[L.N_REJECTED]) == (L.BUDGET, 8, 3, 5)
    compare_with_model("se3", dict(ok=ok, scalars=scalars, trace=trace, state=lm.state.cpu().numpy()), model)


def test_not_positive_definite():
    """f_alpha = -1e6 takes Lambda's diagonal far below zero: the factorization fails, the decision sets status 2,
    slampp_hip_sync reports NOT_POSDEF, the state keeps its bits and later rounds change nothing."""
    lm = make_lm("se3")
    start = lm.state.clone()
    lm.Begin(-1e6, 0.0, 0.0, 20, 10)
    lm.Iterate(2)
    ok, scalars, trace = lm.Sync()
    assert ok is False and scalars[L.STATUS] == L.NOT_POSDEF and scalars[L.ALPHA] == -1e6
    assert (scalars[L.N_ROUNDS], scalars[L.N_ACCEPTED], scalars[L.N_REJECTED], scalars[L.ACCEPTED], scalars[L.ROUNDS_LEFT]) == (1, 0, 0, 0, 20)
    assert len(trace) == 1 and trace[0, L.T_STATUS] == L.NOT_POSDEF and torch.equal(lm.state, start)
    lm.Iterate(1)
    ok, scalars_after, trace_after = lm.Sync()
    assert ok is False and torch.equal(lm.state, start)
    assert np.array_equal(scalars_after, scalars, equal_nan=True) and np.array_equal(trace_after, trace, equal_nan=True)


@pytest.mark.parametrize("kind", M.KINDS)
def test_against_the_reference(kind):
    """tests/golden/lm/: the reference's CNonlinearSolver_Lambda_LM on the same graph from the same state, Optimize(n_max,
    f_min_dx_norm) for n_max = 1 .. 8, with the anchor its system made (recorded in the fixture).  Here Begin(.., n_max, 10) and
    Iterate(n_max + 10): as many solves as the reference counted, and chi^2 and the state no further from the reference's than
    the model is (its exact Jacobians against the reference's forward differences, carried through the loop: up to 6.7e-8 in
    chi^2 on SE(3), 3.3e-6 in the BA state) plus the tolerance of the comparison with the model.  SE(2) has closed-form
    Jacobians on both sides and is within the tolerance itself.  Optimize(3) on SE(3) is the test of the budget: two steps
    accepted, six rejected and granted an iteration each, the ninth solve accepted, status 3.  BA converges in its fifth round;
    past that point rho is 0 / 0 on both sides and nothing is compared (n_max = 6 .. 8 are the same five rounds here)."""
    ref, runs, tol = L.load_reference(kind), L.reference_runs(kind), L.tolerance(kind)
    lm = make_lm(kind, unary=ref["unary"])
    start = dev(lm.graph.fx["state"])
    for n_max, model in enumerate(runs, 1):
        lm.state.copy_(start)
        ok, scalars, trace = lm.Optimize(n_max, float(ref["f_min_dx_norm"]), L.TAU, 0.0, 10)
        sm = model["scalars"]
        counters = [L.STATUS, L.N_ROUNDS, L.N_ACCEPTED, L.N_REJECTED, L.ROUNDS_LEFT, L.EXTRA_LEFT]
        assert ok and np.array_equal(scalars[counters], sm[counters]), (n_max, scalars, sm)
        assert np.array_equal(trace[:, L.T_ACCEPTED], model["trace"][:, L.T_ACCEPTED])
        if kind == "ba" and n_max > 5:
            assert scalars[L.STATUS] == L.CONVERGED and scalars[L.N_ROUNDS] == 5
            continue
        assert scalars[L.N_ROUNDS] == ref["n_iterations"][n_max - 1]
        chi2_ref, state_ref = float(ref["chi2"][n_max - 1]), ref["states"][n_max - 1]
        state = lm.state.cpu().numpy()
        gap_chi2, model_chi2 = abs(scalars[L.LAST_ERROR] - chi2_ref) / chi2_ref, abs(sm[L.LAST_ERROR] - chi2_ref) / chi2_ref
        scale = np.abs(state_ref).max()
        gap_state, model_state = np.abs(state - state_ref).max() / scale, np.abs(model["state"] - state_ref).max() / scale
        print(f"lm {kind} Optimize({n_max}): {int(scalars[L.N_ROUNDS])} solves; from the reference: chi2 {gap_chi2:.2e} (the model {model_chi2:.2e}), "
              f"state {gap_state:.2e} (the model {model_state:.2e})")
        if kind == "se2":
            assert gap_chi2 <= tol["chi2"] and gap_state <= tol["state"]
        assert gap_chi2 <= model_chi2 + tol["chi2"] and gap_state <= model_state + tol["state"]
    if kind == "se3":
        s3 = runs[2]["scalars"]
        assert (s3[L.STATUS], s3[L.N_ROUNDS], s3[L.N_ACCEPTED], s3[L.N_REJECTED]) == (L.BUDGET, 9, 3, 6)


# ---- refusals ----

def test_refusals():
    lm, ba = make_lm("se3"), make_lm("ba")
    lib, s, p = lm._lib, lm._solver, lm._problem
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    q = buf.data_ptr()

    def refused(rc, msg, solver=s, code=ERR_INVALID):
        assert (rc, solver._error()) == (code, msg)

    def with_field(name, value, msg, holder=p, which=lm, code=ERR_INVALID):
        """Both entry points refuse the problem of ``which`` while ``holder`` (the problem, one of its sets or ranges) has the value."""
        saved = getattr(holder, name)
        if isinstance(saved, C._Pointer):               # (a view of the field, which would follow it to NULL: a pointer of its own)
            saved = C.cast(saved, type(saved))
        setattr(holder, name, value)
        try:
            refused(lib.slampp_hip_lm_iterate_device_async(C.byref(which._problem), 1), msg, which._solver, code)
            refused(lib.slampp_hip_lm_begin_device_async(C.byref(which._problem), 1.0, 0.0, 0.0, 5, 10), msg, which._solver, code)
        finally:
            setattr(holder, name, saved)
    before = lm.scalars_dev.clone()
    assert lib.slampp_hip_lm_iterate_device_async(None, 1) == ERR_INVALID
    saved, p.p_solver = p.p_solver, None                # (no handle to leave a text with: the code alone)
    assert lib.slampp_hip_lm_iterate_device_async(C.byref(p), 1) == ERR_INVALID
    assert lib.slampp_hip_lm_begin_device_async(C.byref(p), 1.0, 0.0, 0.0, 5, 10) == ERR_INVALID
    p.p_solver = saved
    for n_rounds in (0, -3):
        refused(lib.slampp_hip_lm_iterate_device_async(C.byref(p), n_rounds), "lm: n_rounds is not positive")
    for name in ("p_sets", "p_ranges", "p_state_dev", "p_trial_dev", "p_values_dev", "p_eta_dev", "p_dx_dev", "p_lm_dev", "p_chi_parts_dev"):
        with_field(name, None, "lm: null pointer")
    for n_sets in (0, 9):
        with_field("n_sets", n_sets, "lm: between 1 and SLAMPP_HIP_LM_MAX_SETS edge sets")
    edge_set = lm._sets[0]
    for name in ("p_measurement_dev", "p_sigma_inv_dev", "p_J0_dev", "p_J1_dev", "p_error_dev"):
        with_field(name, None, "lm: null pointer", edge_set)
    with_field("p_assembly", None, "lm: an edge set's assembly is null or belongs to another solver", edge_set)
    with_field("p_assembly", ba.graph.asm._a, "lm: an edge set's assembly is null or belongs to another solver", edge_set)
    for code in (EDGE_SE2, EDGE_P2C_XYZ, 0, 7):
        with_field("n_edge_type", code, "lm: an edge type does not fit its assembly", edge_set)
    with_field("p_params_dev", None, "lm: null pointer", ba._sets[0], ba)
    # vertex ranges: a gap, an overlap, beyond the end, the wrong type for the block dimension
    n = lm.graph.n_bcols
    vertex_range = lm._ranges[0]
    cover = "lm: the vertex ranges do not cover the block columns exactly once"
    with_field("n_last_vertex", n - 1, cover, vertex_range)
    with_field("n_first_vertex", 1, cover, vertex_range)
    with_field("n_last_vertex", n + 1, cover, vertex_range)
    with_field("n_ranges", 0, cover)
    with_field("n_first_vertex", int(ba.graph.fx["n_cams"]) - 1, cover, ba._ranges[1], ba)    # the two ranges overlap
    with_field("n_vertex_type", 5, "lm: unknown vertex type", vertex_range)
    wrong = "lm: a block column does not have the dimension of its vertex range's type"
    with_field("n_vertex_type", VERTEX_SE2, wrong, vertex_range)
    with_field("n_vertex_type", VERTEX_SE3, wrong, ba._ranges[1], ba)
    overlap = "lm: state, trial and dx overlap"
    with_field("p_trial_dev", lm.state.data_ptr() + 8, overlap)
    with_field("p_dx_dev", lm.state.data_ptr(), overlap)
    with_field("p_dx_dev", lm.trial.data_ptr() + 8 * (lm.graph.n_scalars - 1), overlap)
    with_field("n_unary_vertex", n, "lm: the unary vertex is not a block column")
    # the building blocks
    h = s._h
    assert lib.slampp_hip_edge_errors_device_async(None, EDGE_SE3, q, q, None, q) == ERR_INVALID
    for args in ((None, q, None, q), (q, None, None, q), (q, q, None, None)):
        refused(lib.slampp_hip_edge_errors_device_async(lm.graph.asm._a, EDGE_SE3, *args), "lm: null pointer")
    refused(lib.slampp_hip_edge_errors_device_async(lm.graph.asm._a, EDGE_SE2, q, q, None, q), "lm: an edge type does not fit its assembly")
    refused(lib.slampp_hip_apply_damping_scalar_device_async(h, None, q, 1.0, 0, n), "lm: null pointer")
    refused(lib.slampp_hip_apply_damping_scalar_device_async(h, q, None, 1.0, 0, n), "lm: null pointer")
    for first, last in ((-1, n), (0, n + 1), (5, 4)):
        refused(lib.slampp_hip_apply_damping_scalar_device_async(h, q, q, 1.0, first, last), "lm: bad vertex range")
    assert lib.slampp_hip_lm_initial_damping_device_async(None, 1, 1.0, q) == ERR_INVALID
    for args in ((None, q, q), (q, None, q), (q, q, None)):
        refused(lib.slampp_hip_lm_gain_device_async(h, *args), "lm: null pointer")
        refused(lib.slampp_hip_lm_commit_device_async(h, *args), "lm: null pointer")
    refused(lib.slampp_hip_lm_commit_device_async(h, q, q + 8 * 512, q + 8 * 513), overlap)
    refused(lib.slampp_hip_lm_decide_device_async(h, None, q, 1, None, 0), "lm: null pointer")
    refused(lib.slampp_hip_lm_decide_device_async(h, q, None, 1, None, 0), "lm: null pointer")
    for n_parts in (0, 9):
        refused(lib.slampp_hip_lm_decide_device_async(h, q, q, n_parts, None, 0), "lm: between 1 and SLAMPP_HIP_LM_MAX_SETS edge sets")
    fresh = CLinearSolver_HIP()
    fresh._set_structure(lm.graph.lam)
    refused(lib.slampp_hip_lm_decide_device_async(fresh._h, q, q, 1, None, 0), "lm: analyze was not called", fresh)
    # landmark shards: a handle with an all-reduce callback
    ba._solver.set_allreduce(lambda ptr, count, stream: 0)
    sharded = "lm: not for a handle that solves with landmark shards or over several devices"
    refused(lib.slampp_hip_lm_iterate_device_async(C.byref(ba._problem), 1), sharded, ba._solver, ERR_UNSUPPORTED)
    refused(lib.slampp_hip_lm_begin_device_async(C.byref(ba._problem), 1.0, 0.0, 0.0, 5, 10), sharded, ba._solver, ERR_UNSUPPORTED)
    ba._solver.set_allreduce(None)
    # nothing was enqueued by any of them
    assert s.sync() and torch.equal(lm.scalars_dev, before) and not bool(buf.any())
    # an assembly that another structure has outdated
    s._set_structure(ba.graph.lam)
    refused(lib.slampp_hip_lm_iterate_device_async(C.byref(p), 1), "lm: analyze was not called")
    s.SymbolicDecomposition_Blocky(ba.graph.lam)
    refused(lib.slampp_hip_lm_iterate_device_async(C.byref(p), 1), "lm: set_structure was called after an assembly was created")
