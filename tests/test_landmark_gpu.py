"""The pose-landmark and stereo edges (SLAMPP_HIP_EDGE_POSE_LANDMARK_2D, _POSE_LANDMARK_3D, _P2SC_XYZ) on the GPU, through every
layer: slampp_hip_linearize_device_async and slampp_hip_edge_errors_device_async, into slampp_hip_assemble_sets_device_async
beside a pose-pose set, the Gauss-Newton loop on the device and the LM loop decided there -- on the fixtures of
tests/golden/landmark/ (30 SE(2) poses + 12 landmarks; 15 landmarks + 25 SE(3) poses, the landmarks first, so that every
landmark edge is flipped with d0 != d1; 6 stereo cameras x 40 points in Schur mode).

Values are judged against the exact model of tests/landmark_model.py: 1e-10, rel-inf of the largest entry of each array over
the edge set, as in tests/test_linearize_gpu.py.  The reference (the fixtures) is the yardstick for conventions: its errors
and its 2D Jacobians (closed forms, the range clamp included) to the same 1e-10; its 3D and stereo Jacobians are forward
differences, and the kernel may be as far from them as the model is plus 1e-10.  The LM loops are held to
max(1e-10, 100 x sensitivity), the sensitivity being the Cholesky-versus-LU spread of the model's own loop on the fixture,
measured where the test runs (landmark_model.sensitivity; DESIGN.md section 4.12 records what it was)."""
import numpy as np
import pytest
import torch

import landmark_model as L
import lm_model as LM
import robust_model as R
from golden_util import rel_inf
from slam_plus_plus_amd import synth
from slam_plus_plus_amd import hip_solver as H
from slam_plus_plus_amd.hip_solver import (CLambdaAssembly_HIP, CLevenbergMarquardt_HIP, CLinearSolver_HIP, CLinearSolver_Schur_HIP,
                                           EDGE_P2C_XYZ, EDGE_P2SC_XYZ, EDGE_POSE_LANDMARK_2D, EDGE_POSE_LANDMARK_3D, EDGE_SE2, EDGE_SE3,
                                           ERR_INVALID, LINEARIZE_TILE_EDGES, VERTEX_EUCLIDEAN, VERTEX_SE2, VERTEX_SE3,
                                           Refresh_Lambda_sets_device)

pytestmark = pytest.mark.gpu
M = L.M
TOL = 1e-10
EDGE_TYPE = {"se2": EDGE_SE2, "se3": EDGE_SE3, "lm2d": EDGE_POSE_LANDMARK_2D, "lm3d": EDGE_POSE_LANDMARK_3D, "stereo": EDGE_P2SC_XYZ}
VERTEX_TYPE = {"se2": VERTEX_SE2, "se3": VERTEX_SE3, "euclidean": VERTEX_EUCLIDEAN}
SENTINEL = -7.25e300
N_GUARD = 16

assert (EDGE_POSE_LANDMARK_2D, EDGE_POSE_LANDMARK_3D, EDGE_P2SC_XYZ) == (5, 6, 7) and LINEARIZE_TILE_EDGES == 64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def guarded(n):
    """n doubles followed by sentinels."""
    return torch.full((n + N_GUARD,), SENTINEL, dtype=torch.float64, device="cuda")


def guard_intact(t, n):
    return bool((t[n:] == SENTINEL).all())


def col_major(J):
    return np.ascontiguousarray(np.transpose(J, (0, 2, 1)))


class EdgeSet:
    """One edge set of a graph on the device: its assembly handle over the edge list given and the input arrays."""

    def __init__(self, graph, s, n_tile=1, n_edges=None):
        self.kind, self.host = s["kind"], s
        self.d0, self.d1, self.rd = L.EDGE_SHAPES[self.kind]
        v0, v1 = np.tile(s["v0"], n_tile), np.tile(s["v1"], n_tile)
        self.n_edges = n = len(v0) if n_edges is None else n_edges
        self.asm = CLambdaAssembly_HIP(graph.solver, graph.lam, v0[:n], v1[:n], self.rd)
        self.z = dev(np.tile(s["z"], (n_tile, 1))[:n])
        self.sigma_inv = dev(col_major(np.tile(s["sigma_inv"], (n_tile, 1, 1))[:n]))
        self.params = None if s["params"] is None else dev(s["params"])
        self.params_ptr = 0 if self.params is None else self.params.data_ptr()
        self.sizes = (n * self.rd * self.d0, n * self.rd * self.d1, n * self.rd)

    def outputs(self):
        return tuple(guarded(k) for k in self.sizes)

    def linearize(self, state, out=None):
        """(J0, J1, err) as the call left them, each followed by its sentinels (enqueue-only where ``out`` is given)."""
        J0, J1, err = out or self.outputs()
        if out is None:
            torch.cuda.synchronize()
        self.asm.Linearize_device(EDGE_TYPE[self.kind], state.data_ptr(), self.z.data_ptr(), J0.data_ptr(), J1.data_ptr(), err.data_ptr(),
                                  self.params_ptr)
        return J0, J1, err

    def as_model(self, J0, J1, err):
        """The kernel's arrays in the model's shapes ([E, rd, d] row-major, [E, rd])."""
        n = self.n_edges
        return (J0[:self.sizes[0]].cpu().numpy().reshape(n, self.d0, self.rd).transpose(0, 2, 1),
                J1[:self.sizes[1]].cpu().numpy().reshape(n, self.d1, self.rd).transpose(0, 2, 1),
                err[:self.sizes[2]].cpu().numpy().reshape(n, self.rd))


class Graph:
    """A fixture on the device: the solver, Lambda's structure (of all the fixture's edges) and its edge sets, the landmark
    or stereo set last (``main``), over all its edges or the regular ones."""

    def __init__(self, name, regular_only=False):
        self.name, self.fx = name, L.load_fixture(name)
        fx = self.fx
        self.host_sets = L.edge_sets(name, regular_only)
        every = L.edge_sets(name, False)
        self.dims = np.diff(fx["cumsum"])
        self.lam = synth.structure_from_edges(self.dims, np.concatenate([s["v0"] for s in every]), np.concatenate([s["v1"] for s in every]))
        if name == "stereo":
            self.lam.n_matrix_cut = int(fx["n_poses"])
            self.solver = CLinearSolver_Schur_HIP()
        else:
            self.solver = CLinearSolver_HIP()
        self.sets = [EdgeSet(self, s) for s in self.host_sets]
        self.main = self.sets[-1]
        self.state = dev(fx["state"])
        self.n_scalars, self.n_bcols = int(fx["cumsum"][-1]), len(self.dims)
        self.ranges = [(VERTEX_TYPE[k], first, last) for k, first, last in L.vertex_ranges(name, fx)]

    def linearize(self):
        out = self.main.linearize(self.state)
        assert self.solver.sync()
        return out


_graphs = {}


def graph(name, regular_only=False):
    """One Graph per fixture and edge choice, shared by the tests that only read it."""
    if (name, regular_only) not in _graphs:
        _graphs[name, regular_only] = Graph(name, regular_only)
    return _graphs[name, regular_only]


@pytest.fixture(scope="module", params=L.NAMES)
def linearized(request):
    g = graph(request.param)
    return g, g.linearize()


# ---- linearize ----

def test_against_the_model(linearized):
    g, out = linearized
    J0, J1, err = g.main.as_model(*out)
    _, err_m, J0_m, J1_m = L.fixture_model(g.name)
    assert rel_inf(err, err_m) < TOL
    assert rel_inf(J0, J0_m) < TOL
    assert rel_inf(J1, J1_m) < TOL
    if g.name == "lm2d":       # without the clamped edges' entries of 1e5, and those on their own
        assert rel_inf(J0[:-3], J0_m[:-3]) < TOL and rel_inf(J1[:-3], J1_m[:-3]) < TOL
        assert rel_inf(J0[-3:], J0_m[-3:]) < TOL and rel_inf(J1[-3:], J1_m[-3:]) < TOL
        assert not np.isnan(J0).any() and not np.isnan(J1).any() and not np.isnan(err).any()
    assert all(guard_intact(t, t.numel() - N_GUARD) for t in out)


def test_against_the_reference(linearized):
    g, out = linearized
    J0, J1, err = g.main.as_model(*out)
    _, _, J0_m, J1_m = L.fixture_model(g.name)
    fx = g.fx
    assert rel_inf(err, fx["err"]) < TOL
    for J, J_m, J_ref in ((J0, J0_m, fx["J0"]), (J1, J1_m, fx["J1"])):
        if g.name == "lm2d":
            assert rel_inf(J, J_ref) < TOL and rel_inf(J[:-3], J_ref[:-3]) < TOL
        else:   # forward differences on the reference's side: no further from them than the exact derivative is
            assert np.abs(J - J_ref).max() <= np.abs(J_m - J_ref).max() + TOL * np.abs(J_m).max()


def test_same_bits_twice(linearized):
    g, out = linearized
    again = g.linearize()
    assert all(torch.equal(a, b) for a, b in zip(out, again))


def test_edge_errors_has_the_bits_of_linearize(linearized):
    g, (_, _, err) = linearized
    s = g.main
    only = guarded(s.sizes[2])
    torch.cuda.synchronize()
    g.solver._check(g.solver._lib.slampp_hip_edge_errors_device_async(s.asm._a, EDGE_TYPE[s.kind], g.state.data_ptr(), s.z.data_ptr(),
                                                                   s.params_ptr or None, only.data_ptr()))
    assert g.solver.sync()
    assert torch.equal(only, err) and guard_intact(only, s.sizes[2]) and not bool((only[:s.sizes[2]] == SENTINEL).any())


_tiled = {}


def tiled(name):
    """The fixture's landmark / stereo edge list several times over, 130 edges or more (lm2d 3 x 55 = 165, stereo 2 x 119 =
    238: two full store tiles and a ragged one at least), linearized once."""
    if name not in _tiled:
        g = graph(name)
        n_tile = -(-130 // len(g.host_sets[-1]["v0"]))
        s = EdgeSet(g, g.host_sets[-1], n_tile)
        out = s.linearize(g.state)
        assert g.solver.sync() and s.n_edges >= 130
        J0, J1, err = s.as_model(*out)
        _, err_m, J0_m, J1_m = L.fixture_model(name)
        assert rel_inf(J0, np.tile(J0_m, (n_tile, 1, 1))) < TOL and rel_inf(J1, np.tile(J1_m, (n_tile, 1, 1))) < TOL
        assert rel_inf(err, np.tile(err_m, (n_tile, 1))) < TOL
        _tiled[name] = dict(n_tile=n_tile, out=out)
    return _tiled[name]


@pytest.mark.parametrize("n_edges", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("name", ["stereo", "lm2d"])
def test_edge_counts_around_the_store_tile(name, n_edges):
    """The tile rows are 19 / 9 / 3 doubles (stereo) and 7 / 5 / 3 (lm2d): the first n edges in a call of their own have the
    bits they have in the call on all, and nothing is written behind them."""
    full = tiled(name)
    assert all(guard_intact(t, t.numel() - N_GUARD) for t in full["out"])
    g = graph(name)
    short = EdgeSet(g, g.host_sets[-1], full["n_tile"], n_edges)
    out = short.linearize(g.state)
    assert g.solver.sync()
    for a, b, n in zip(out, full["out"], short.sizes):
        assert torch.equal(a[:n], b[:n]) and guard_intact(a, n)


# ---- into the assembly ----

def unary_10(g):
    """(vertex, factor, error): 10 I on the first pose; none in Schur mode."""
    if g.name == "stereo":
        return -1, None, None
    v = int(g.fx["n_first_pose"])
    d = int(g.dims[v])
    return v, 10.0 * np.eye(d), np.zeros(d)


def assemble_sets(g, outs, values, eta, unary):
    Refresh_Lambda_sets_device([s.asm for s in g.sets], [(J0.data_ptr(), J1.data_ptr(), s.sigma_inv.data_ptr(), err.data_ptr(), 0)
                                                         for s, (J0, J1, err) in zip(g.sets, outs)], values.data_ptr(), eta.data_ptr(), *unary)


@pytest.mark.parametrize("name", L.NAMES)
def test_into_the_assembly(name):
    """Every set linearized on the device and assembled in one call with the unary factor (lm2d, lm3d: the pose-pose set and
    the landmark set, the latter's edges all flipped with d0 != d1 on lm3d; stereo: one set on the Schur handle), against the
    model's dense Lambda and eta."""
    g = graph(name, True)
    fx, unary = g.fx, unary_10(g)
    values = torch.full((g.lam.values.shape[0],), float("nan"), dtype=torch.float64, device="cuda")
    eta = torch.full((g.n_scalars,), float("nan"), dtype=torch.float64, device="cuda")
    outs = [s.outputs() for s in g.sets]
    torch.cuda.synchronize()
    for s, out in zip(g.sets, outs):
        s.linearize(g.state, out)
    assemble_sets(g, outs, values, eta, unary)
    assert g.solver.sync()
    lins = L.linearize_sets(g.host_sets, fx["state"], fx["cumsum"])
    lam_dense, eta_dense = L.dense_system(fx["cumsum"], g.host_sets, lins, *(unary if unary[0] >= 0 else ()))
    assert rel_inf(eta.cpu().numpy(), eta_dense) < TOL
    g.lam.values = values.cpu().numpy()
    assert rel_inf(np.triu(g.lam.to_scipy().toarray()), np.triu(lam_dense)) < TOL
    if name == "lm3d":
        assert (g.host_sets[-1]["v0"] > g.host_sets[-1]["v1"]).all()


# ---- the loops ----

@pytest.mark.parametrize("name", L.NAMES)
def test_gauss_newton_loop_on_the_device(name):
    """Five iterations of linearize (every set) -> assemble_sets -> (damp) -> factor_solve -> plus (every vertex range) -> chi2,
    nothing copied to the host inside one, in the form of tests/test_linearize_gpu.py: the entering state and the dx of every
    iteration are kept in device arrays and judged afterwards, each iteration from its own entering state -- the model's
    Jacobians, a dense Lambda and eta, numpy's solution.  lm2d, lm3d: sparse mode, the unary factor 10 I on the first pose.
    stereo: Schur mode, no prior, Lambda damped by 100 on its diagonal."""
    g = graph(name, True)
    fx, n, nv, n_it = g.fx, g.n_scalars, g.lam.values.shape[0], 5
    unary = unary_10(g)
    damping = 100.0 if name == "stereo" else 0.0
    state = g.state.clone()
    outs = [s.outputs() for s in g.sets]
    values, eta = torch.zeros(nv, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
    entering, steps = torch.zeros((n_it, n), dtype=torch.float64, device="cuda"), torch.zeros((n_it, n), dtype=torch.float64, device="cuda")
    chi2 = torch.zeros((n_it + 1, len(g.sets)), dtype=torch.float64, device="cuda")
    stream = torch.cuda.ExternalStream(g.solver.stream())
    torch.cuda.synchronize()
    for k in range(n_it + 1):
        for i, (s, out) in enumerate(zip(g.sets, outs)):
            s.linearize(state, out)
            s.asm.Chi2_device(s.sigma_inv.data_ptr(), out[2].data_ptr(), 0, chi2[k, i].data_ptr())
        if k == n_it:
            break
        assemble_sets(g, outs, values, eta, unary)
        if damping:
            g.solver.apply_damping_device_async(values.data_ptr(), damping, 0, g.n_bcols)
        g.solver.factor_solve_device_async(values.data_ptr(), eta.data_ptr())
        with torch.cuda.stream(stream):
            entering[k].copy_(state)
            steps[k].copy_(eta)
        for vertex_type, first, last in g.ranges:
            g.solver.State_Plus_device(vertex_type, first, last, state.data_ptr(), eta.data_ptr(), state.data_ptr())
    assert g.solver.sync()
    torch.cuda.synchronize()
    entering, steps, chi2 = entering.cpu().numpy(), steps.cpu().numpy(), chi2.cpu().numpy()
    assert np.array_equal(entering[0], fx["state"]) and len(g.ranges) == 2
    for k in range(n_it):
        lins = L.linearize_sets(g.host_sets, entering[k], fx["cumsum"])
        lam_dense, eta_dense = L.dense_system(fx["cumsum"], g.host_sets, lins, *(unary if unary[0] >= 0 else ()))
        dx = np.linalg.solve(lam_dense + damping * np.eye(n), eta_dense)
        print(f"landmark_{name}: iteration {k}: dx from numpy's by {rel_inf(steps[k], dx):.3g}")
        assert rel_inf(steps[k], dx) < TOL, (k, rel_inf(steps[k], dx))
        for i, (s, lin) in enumerate(zip(g.host_sets, lins)):
            assert abs(chi2[k, i] - M.chi2(lin[1], s["sigma_inv"])) < TOL * chi2[k, i]
    chi2 = chi2.sum(1)
    print(f"landmark_{name}: chi2 over the iterations {chi2}")
    # the rule of tests/test_linearize_gpu.py and its reason: the Jacobians are dh / de, so the loop's fixed point is not
    # chi^2's stationary point and chi^2 wanders around it at second order in the residual; no step raises it by more than 1 %
    assert chi2[n_it] < chi2[0], chi2
    assert all(chi2[k + 1] <= 1.01 * chi2[k] for k in range(n_it)), chi2
    assert all(guard_intact(t, t.numel() - N_GUARD) for out in outs for t in out)


def make_lm(name, robust=None):
    """CLevenbergMarquardt_HIP over the fixture's sets (the regular edges) and vertex ranges, a graph of its own; ``robust``: a
    robust_model.Spec on the landmark set."""
    g = Graph(name, True)
    sets = [dict(assembly=s.asm, edge_type=EDGE_TYPE[s.kind], measurement=s.z, sigma_inv=s.sigma_inv, params=s.params) for s in g.sets]
    if robust is not None:
        sets[-1]["robust"] = dict(robust._asdict())
    lm = CLevenbergMarquardt_HIP(g.solver, g.lam, sets, g.ranges, g.fx["state"], L.unary_of(name, g.fx), 64)
    lm.graph = g
    return lm


@pytest.mark.parametrize("name", sorted(L.LOOPS))
def test_lm_loop_against_the_model(name):
    """lm2d: the SE(2) set and the landmark set, the ranges SE2 and EUCLIDEAN, 10 rounds enqueued, converged (|dx| <= 1e-4) in
    the eighth.  stereo: Schur mode, 8 rounds.  The accept flags and the status of every round are the model's; alpha, chi^2,
    rho, |dx| and the final state within max(1e-10, 100 x sensitivity), printed."""
    n_rounds, f_min_dx_norm = L.LOOPS[name]
    model, tol = L.fixture_run(name), L.tolerance(name)
    print(f"landmark_{name}: sensitivity {L.sensitivity(name)}")
    lm = make_lm(name)
    lm.Begin(0.0, LM.TAU, f_min_dx_norm)
    lm.Iterate(n_rounds)
    ok, s, t = lm.Sync()
    tm, sm = model["trace"], model["scalars"]
    assert ok and t.shape == tm.shape
    k = LM.compared_rounds(model)
    assert k >= 5
    for col in (LM.T_ACCEPTED, LM.T_STATUS, LM.T_NU):
        assert np.array_equal(t[:, col], tm[:, col]), (col, t[:, col], tm[:, col])
    ints = [LM.NU, LM.STATUS, LM.N_ROUNDS, LM.N_ACCEPTED, LM.N_REJECTED, LM.ROUNDS_LEFT, LM.EXTRA_LEFT, LM.MIN_DX_NORM, LM.N_RECORDS]
    assert np.array_equal(s[ints], sm[ints]), (s, sm)
    for q, col in (("alpha", LM.T_ALPHA), ("chi2", LM.T_ERROR), ("chi2", LM.T_LAST_ERROR), ("rho", LM.T_RHO), ("dx_norm", LM.T_DX_NORM)):
        gap = np.abs(t[:k, col] - tm[:k, col]) / np.abs(tm[:k, col])
        print(f"landmark_{name}: {q} (trace column {col}) from the model by {gap.max():.3g}, tolerance {tol[q]:.3g}")
        assert np.all(gap <= tol[q]), (q, col, gap)
    assert abs(s[LM.LAST_ERROR] - sm[LM.LAST_ERROR]) <= tol["chi2"] * sm[LM.LAST_ERROR]
    gap = np.abs(lm.state.cpu().numpy() - model["state"]).max() / np.abs(model["state"]).max()
    print(f"landmark_{name}: the final state from the model by {gap:.3g}, tolerance {tol['state']:.3g}")
    assert gap <= tol["state"]


def device_view(ptr, n):
    """n doubles of device memory at ``ptr`` as a tensor (no copy)."""
    class View:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2}
    return torch.as_tensor(View(), device="cuda")


def test_lm_loop_with_a_robust_landmark_set():
    """Huber on |err| / 0.2 (ROBUST_MODE_REFERENCE) on the landmark set of lm2d: the loop enqueues and syncs cleanly; the
    weights the handle holds are robust_model's on the errors of the last linearization (at the state that entered the last
    round), and the weights of the final state's errors are robust_model's too."""
    spec = R.Spec(R.HUBER, R.ERROR_NORM, R.REFERENCE, 0.2, 1.345)
    lm = make_lm("lm2d", spec)
    g = lm.graph
    s, n = g.main, g.main.n_edges
    lm.Begin(0.0, LM.TAU, 0.0)
    lm.Iterate(5)
    ok, scalars, trace = lm.Sync()
    assert ok and scalars[LM.N_ROUNDS] == 5 and scalars[LM.N_ACCEPTED] >= 1 and np.isfinite(trace).all()
    entering = lm.state.cpu().numpy()
    lm.Iterate(1)
    ok, scalars, _ = lm.Sync()
    assert ok and scalars[LM.N_ROUNDS] == 6 and np.isfinite(scalars).all()
    w = device_view(s.asm.Robust_Weights_ptr(), n).cpu().numpy()
    host = g.host_sets[-1]
    _, err_m, _, _ = L.linearize("lm2d", entering, g.fx["cumsum"], host["v0"], host["v1"], host["z"])
    w_m = R.weights(spec, err_m)
    assert np.abs(w - w_m).max() < TOL and 0 < (w_m < 1).sum() < n
    out = s.linearize(lm.state)
    s.asm.Robust_Weights_device(s.sigma_inv.data_ptr(), out[2].data_ptr())
    assert g.solver.sync()
    w = device_view(s.asm.Robust_Weights_ptr(), n).cpu().numpy()
    w_m = R.weights(spec, s.as_model(*out)[2])
    assert np.abs(w - w_m).max() < TOL and 0 < (w_m < 1).sum() < n


# ---- refusals ----

def test_refusals():
    lm2d, lm3d, stereo = graph("lm2d"), graph("lm3d"), graph("stereo")
    lib = lm2d.solver._lib
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()

    def refused(g, rc, msg):
        assert (rc, g.solver._error()) == (ERR_INVALID, msg)
    dims, fit = "linearize: the edge type's dimensions are not this assembly's", "lm: an edge type does not fit its assembly"
    # (assembly, the types whose dimensions are not its own)
    cases = [(lm2d, lm2d.main, (EDGE_SE2, EDGE_POSE_LANDMARK_3D, EDGE_P2SC_XYZ, EDGE_P2C_XYZ)),
             (lm2d, lm2d.sets[0], (EDGE_POSE_LANDMARK_2D, EDGE_POSE_LANDMARK_3D, EDGE_P2SC_XYZ)),
             (lm3d, lm3d.main, (EDGE_SE3, EDGE_POSE_LANDMARK_2D, EDGE_P2C_XYZ)),
             (lm3d, lm3d.sets[0], (EDGE_POSE_LANDMARK_2D, EDGE_POSE_LANDMARK_3D, EDGE_P2SC_XYZ)),
             (stereo, stereo.main, (EDGE_SE3, EDGE_POSE_LANDMARK_2D, EDGE_P2C_XYZ))]     # P2C_XYZ: rd 3 != 2
    for g, s, codes in cases:
        for code in codes:
            refused(g, lib.slampp_hip_linearize_device_async(s.asm._a, code, p, p, p, p, p, p), dims)
            refused(g, lib.slampp_hip_edge_errors_device_async(s.asm._a, code, p, p, p, p), fit)
        for code in (4, 0, 8, -1):                        # 4 stays unassigned; the unknown type is refused before the dimensions
            refused(g, lib.slampp_hip_linearize_device_async(s.asm._a, code, p, p, p, p, p, p), "linearize: unknown edge type")
            refused(g, lib.slampp_hip_edge_errors_device_async(s.asm._a, code, p, p, p, p), fit)
    refused(stereo, lib.slampp_hip_linearize_device_async(stereo.main.asm._a, EDGE_P2SC_XYZ, p, p, None, p, p, p),
            "linearize: SLAMPP_HIP_EDGE_P2SC_XYZ needs p_params_dev")
    refused(stereo, lib.slampp_hip_edge_errors_device_async(stereo.main.asm._a, EDGE_P2SC_XYZ, p, p, None, p), "lm: null pointer")
    # the loop's entry points say the same of a set
    lm = make_lm("stereo")
    import ctypes as C
    saved = lm._sets[0].p_params_dev
    lm._sets[0].p_params_dev = None
    refused(lm.graph, lib.slampp_hip_lm_begin_device_async(C.byref(lm._problem), 1.0, 0.0, 0.0, 5, 10), "lm: null pointer")
    refused(lm.graph, lib.slampp_hip_lm_iterate_device_async(C.byref(lm._problem), 1), "lm: null pointer")
    lm._sets[0].p_params_dev = saved
    for code in (EDGE_P2C_XYZ, EDGE_POSE_LANDMARK_2D, 4):
        lm._sets[0].n_edge_type = code
        refused(lm.graph, lib.slampp_hip_lm_iterate_device_async(C.byref(lm._problem), 1), fit)
    lm._sets[0].n_edge_type = EDGE_P2SC_XYZ
    # nothing was enqueued by any of them
    assert all(g.solver.sync() for g in (lm2d, lm3d, stereo, lm.graph)) and not bool(buf.any())
