"""Robust kernels on the device (csrc/robust.hip, csrc/capi_robust.hip, and their use in csrc/capi_lm.hip) on the GPU, against the
numpy model of tests/robust_model.py and the reference's own figures in tests/golden/robust/.

The three kernels are compared with the model to the project's kernel-against-model tolerance, 1e-10 relative, on SE(2), SE(3)
and camera-point edge sets (rd = 3, 6, 2) of 1, 63, 64, 65 and 130 edges, for the four loss functions and the three bases, with
planted edges whose s is exactly 0, the doubles either side of a, a itself and 1e3 a: there the comparison is exact (Welsch, whose
exp is the library's, aside).  The loops are compared as tests/test_lm_gpu.py compares them: decisions, status and counters
exactly, figures to 100 x the Cholesky-against-LU sensitivity of the same loop in the model and not below 1e-10
(robust_model.tolerance), the final state of the REFERENCE loop no further from the reference's than the model's is, plus that."""
import ctypes as C

import numpy as np
import pytest
import torch

import linearize_model as M
import lm_model as L
import robust_model as R
import test_lm_gpu as T
from slam_plus_plus_amd import hip_solver as H
from slam_plus_plus_amd.hip_solver import CLevenbergMarquardt_HIP, CLinearSolver_HIP, CLinearSolver_Schur_HIP, ERR_INVALID

pytestmark = pytest.mark.gpu
TOL = 1e-10
dev, guarded, guard_intact, SENTINEL = T.dev, T.guarded, T.guard_intact, T.SENTINEL
SCALE = 0.5                                            # (a power of two: s of a planted edge is exact)

# the model's constants are the header's
assert (H.ROBUST_HUBER, H.ROBUST_CAUCHY, H.ROBUST_TUKEY, H.ROBUST_WELSCH) == (R.HUBER, R.CAUCHY, R.TUKEY, R.WELSCH)
assert (H.ROBUST_BASIS_ERROR_NORM, H.ROBUST_BASIS_CHI2, H.ROBUST_BASIS_MAHALANOBIS) == (R.ERROR_NORM, R.CHI2, R.MAHALANOBIS)
assert (H.ROBUST_MODE_REFERENCE, H.ROBUST_MODE_LOSS) == (R.REFERENCE, R.LOSS) and H.ROBUST_DEFAULT_PARAM == R.DEFAULT_PARAM


def set_robust(asm, spec):
    asm.Set_Robust(spec.kernel, spec.basis, spec.mode, spec.scale, spec.param)


def as_dict(spec):
    return dict(spec._asdict())


def device_view(ptr, n):
    """n doubles of device memory at ``ptr`` as a tensor (no copy)."""
    class View:
        __cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2}
    return torch.as_tensor(View(), device="cuda")


def edge_data(n, rd, basis, a, seed):
    """(err [n, rd], sigma_inv [n, rd, rd] symmetric positive definite and not diagonal, planted) with s of about a third of the
    edges beyond a, and planted edges -- zero error, s = the double below a, a, the double above a, 1e3 a, and 1e3 a again in the
    last edge -- as far as n has room; ``planted``: {edge: s}."""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(n, rd, rd))
    omega = A @ np.transpose(A, (0, 2, 1)) + 0.5 * np.eye(rd)
    err = rng.normal(size=(n, rd))
    s = R.basis_argument(basis, SCALE, err, omega)
    target = a * rng.permutation(np.linspace(0.11, 1.44, n))  # a third beyond a, none within 1e-3 a of it at the n used
    err *= (np.sqrt(target / s) if basis == R.CHI2 else target / s)[:, None]
    want = [0.0, np.nextafter(a, 0), a, np.nextafter(a, 2 * a), 1e3 * a]
    planted = {e: v for e, v in enumerate(want) if e < n}
    if n > len(want):
        planted[n - 1] = 1e3 * a
    for e, v in planted.items():
        omega[e], err[e] = np.eye(rd), 0
        if basis == R.CHI2:
            omega[e, 0, 0], err[e, 0] = max(v * SCALE, 1.0 if v == 0 else 0.0), (0.0 if v == 0 else 1.0)   # q = Omega_00 exactly
        else:
            err[e, 0] = v * SCALE                            # |err| = sqrt(err^T err) = v SCALE exactly
    assert np.array_equal(R.basis_argument(basis, SCALE, err, omega)[list(planted)], list(planted.values()))
    return err, omega, planted


def check_weights(got, want, planted, kernel, what):
    assert not np.any(np.isnan(got)), what
    gap = np.abs(got - want)
    assert np.all(gap <= TOL * want + 1e-300), (what, gap.max())
    if kernel != R.WELSCH:
        idx = list(planted)
        assert np.array_equal(got[idx], want[idx]), (what, got[idx], want[idx])
    for e, s in planted.items():
        if s == 0:
            assert got[e] == 1, what


# ---- the three kernels against the model ----

@pytest.mark.parametrize("n_edges", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("kind", M.KINDS)
def test_kernels_against_the_model(kind, n_edges):
    """Every loss function on every basis: the weights into an array given and into the handle's own, twice to the same bits; the
    cost (MAHALANOBIS); the arrays one double off a 16-byte boundary on every other combination (the 8-byte loads)."""
    g = T.Graph(kind, n_edges, n_tile=4)
    rd, n = g.rd, n_edges
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    for i, (kernel, basis) in enumerate((k, b) for k in R.KERNELS.values() for b in R.BASES.values()):
        a = R.DEFAULT_PARAM[kernel]
        spec = R.Spec(kernel, basis, R.REFERENCE, SCALE, a)
        what = (kind, n, kernel, basis)
        err, omega, planted = edge_data(n, rd, basis, a, 100 * n + i)
        off = i % 2
        d_err, d_omega, d_w, d_w2 = guarded(n * rd + 1), guarded(n * rd * rd + 1), guarded(n + 1), guarded(n + 1)
        d_err[off:off + n * rd], d_omega[off:off + n * rd * rd] = dev(err).ravel(), dev(T.col_major(omega)).ravel()
        p_err, p_omega = d_err.data_ptr() + 8 * off, d_omega.data_ptr() + 8 * off
        set_robust(g.asm, spec)
        own = device_view(g.asm.Robust_Weights_ptr(), n)
        torch.cuda.synchronize()
        g.asm.Robust_Weights_device(0 if basis == R.ERROR_NORM else p_omega, p_err, d_w.data_ptr() + 8 * off)
        g.asm.Robust_Weights_device(p_omega, p_err, d_w2.data_ptr() + 8 * off)
        g.asm.Robust_Weights_device(p_omega, p_err, 0)
        assert g.solver.sync()
        want = R.weights(spec, err, omega)
        got = d_w[off:off + n].cpu().numpy()
        check_weights(got, want, planted, kernel, what)
        assert torch.equal(d_w, d_w2) and torch.equal(own, d_w[off:off + n]), what
        assert bool((d_w[:off] == SENTINEL).all()) and bool((d_w[off + n:] == SENTINEL).all()), what
        if kernel == R.TUKEY:
            assert all(got[e] == 0 for e, s in planted.items() if s > a), what
        if kernel == R.WELSCH:
            assert all(0 <= got[e] < 1e-300 for e, s in planted.items() if s > 2 * a), what
        assert n < 60 or abs(np.mean(R.basis_argument(basis, SCALE, err, omega) > a) - 1 / 3) < 0.15, what    # about a third beyond a
        if basis == R.MAHALANOBIS:
            g.asm.Robust_Chi2_device(p_omega, p_err, out.data_ptr())
            g.asm.Robust_Chi2_device(p_omega, p_err, out.data_ptr() + 8)
            assert g.solver.sync()
            cost = R.cost(spec._replace(mode=R.LOSS), err, omega)
            assert abs(float(out[0]) - cost) <= TOL * cost and float(out[0]) == float(out[1]), (what, float(out[0]), cost)


@pytest.mark.parametrize("n_edges", [1, 65, 130])
@pytest.mark.parametrize("kind", M.KINDS)
def test_scale(kind, n_edges):
    """J0, J1 and err times sqrt(w), to the bits of the model's product, with the weights given and with the handle's; nothing
    outside the three arrays is touched.  The arrays on a 16-byte boundary and one double off it."""
    g = T.Graph(kind, n_edges, n_tile=4)
    n, rng = n_edges, np.random.default_rng(n_edges)
    spec = R.Spec(R.CAUCHY, R.MAHALANOBIS, R.LOSS, SCALE, 2.385)
    set_robust(g.asm, spec)
    err, omega, _ = edge_data(n, g.rd, spec.basis, spec.param, 7 * n)
    w = R.weights(spec, err, omega)
    J0, J1 = rng.normal(size=(n, g.d0, g.rd)), rng.normal(size=(n, g.d1, g.rd))     # (any layout: the scaling is per element)
    want = R.scaled(w, J0, J1, err)
    d_w, d_omega = dev(w), dev(T.col_major(omega))
    for off, own in ((0, False), (1, False), (0, True)):
        arrays = []
        for a in (J0, J1, err):
            t = guarded(a.size + 1)
            t[off:off + a.size] = dev(a).ravel()
            arrays.append(t)
        torch.cuda.synchronize()
        if own:
            g.asm.Robust_Weights_device(d_omega.data_ptr(), arrays[2].data_ptr() + 8 * off, 0)
        g.asm.Robust_Scale_device(*(t.data_ptr() + 8 * off for t in arrays), 0 if own else d_w.data_ptr())
        assert g.solver.sync()
        for t, a, x in zip(arrays, (J0, J1, err), want):
            got = t[off:off + a.size].cpu().numpy()
            if own:                                      # (the handle's weights are the device's: 1e-10 from the model's)
                assert np.all(np.abs(got - x.ravel()) <= TOL * np.abs(x.ravel()))
            else:
                assert np.array_equal(got, x.ravel()), (kind, n, off, np.abs(got - x.ravel()).max())
            assert bool((t[:off] == SENTINEL).all()) and bool((t[off + a.size:] == SENTINEL).all())


def test_an_edge_does_not_depend_on_its_neighbours():
    """The first 65 weights of a 130-edge call have the bits of the 65-edge call on the same data."""
    whole, part = T.Graph("se3", 130, n_tile=4), T.Graph("se3", 65, n_tile=4)
    for kernel, basis in ((R.HUBER, R.ERROR_NORM), (R.WELSCH, R.CHI2), (R.TUKEY, R.MAHALANOBIS)):
        spec = R.Spec(kernel, basis, R.REFERENCE, SCALE, R.DEFAULT_PARAM[kernel])
        err, omega, _ = edge_data(130, 6, basis, spec.param, 3)
        d_err, d_omega, a, b = dev(err), dev(T.col_major(omega)), guarded(130), guarded(65)
        torch.cuda.synchronize()
        for g, w in ((whole, a), (part, b)):
            set_robust(g.asm, spec)
            g.asm.Robust_Weights_device(d_omega.data_ptr(), d_err.data_ptr(), w.data_ptr())
            assert g.solver.sync()
        assert torch.equal(a[:65], b[:65]) and guard_intact(a, 130) and guard_intact(b, 65)


# ---- the loops ----

def make_lm(kind, robust, z=None, unary="default", solver_class=None, robust_edges=None):
    """tests/test_lm_gpu.make_lm with a robust kernel (a Spec) on the set, or on the first ``robust_edges`` edges as a set of
    their own before the plain rest."""
    g = T.Graph(kind, solver_class=solver_class)
    if z is not None:
        g.z = dev(z)
    if isinstance(unary, str):
        unary = L.unary_of(kind, g.fx)
    elif unary is not None:
        unary = (unary[0], np.ascontiguousarray(np.asarray(unary[1]).T), unary[2])
    fx, k = g.fx, robust_edges
    if k is None:
        sets = [dict(assembly=g.asm, edge_type=T.EDGE_TYPE[kind], measurement=g.z, sigma_inv=g.sigma_inv, params=g.params,
                     robust=None if robust is None else as_dict(robust))]
    else:
        cut = [H.CLambdaAssembly_HIP(g.solver, g.lam, fx["v0"][c], fx["v1"][c], g.rd) for c in (slice(0, k), slice(k, None))]
        sets = [dict(assembly=cut[0], edge_type=T.EDGE_TYPE[kind], measurement=g.z[:k], sigma_inv=g.sigma_inv[:k], params=g.params,
                     robust=as_dict(robust)),
                dict(assembly=cut[1], edge_type=T.EDGE_TYPE[kind], measurement=g.z[k:], sigma_inv=g.sigma_inv[k:], params=g.params)]
    lm = CLevenbergMarquardt_HIP(g.solver, g.lam, sets, T.vertex_ranges(kind, fx), fx["state"], unary, 64)
    lm.graph, lm.assemblies = g, [s["assembly"] for s in sets]
    return lm


def compare_with_model(what, run, model, tol):
    """tests/test_lm_gpu.compare_with_model with the tolerance given.  ACCEPTED is left out: the model stops at the round that
    sets the status, the device runs the rounds enqueued behind it, which clear the flag; the trace has every decision's."""
    t, tm, s, sm = run["trace"], model["trace"], run["scalars"], model["scalars"]
    assert run["ok"] and t.shape == tm.shape, (what, t.shape, tm.shape)
    for col in (L.T_ACCEPTED, L.T_STATUS, L.T_NU):
        assert np.array_equal(t[:, col], tm[:, col]), (what, col, t[:, col], tm[:, col])
    ints = [L.NU, L.STATUS, L.N_ROUNDS, L.N_ACCEPTED, L.N_REJECTED, L.ROUNDS_LEFT, L.EXTRA_LEFT, L.MIN_DX_NORM, L.N_RECORDS]
    assert np.array_equal(s[ints], sm[ints]), (what, s, sm)
    k = L.compared_rounds(model)
    for q, col in (("alpha", L.T_ALPHA), ("chi2", L.T_ERROR), ("chi2", L.T_LAST_ERROR), ("rho", L.T_RHO), ("dx_norm", L.T_DX_NORM)):
        gap = np.abs(t[:k, col] - tm[:k, col]) / np.abs(tm[:k, col])
        print(f"{what}: {q} (trace column {col}) from the model by {gap.max():.3g}, tolerance {tol[q]:.3g}")
        assert np.all(gap <= tol[q]), (what, q, col, gap)
    assert abs(s[L.LAST_ERROR] - sm[L.LAST_ERROR]) <= tol["chi2"] * sm[L.LAST_ERROR]
    gap = np.abs(run["state"] - model["state"]).max() / np.abs(model["state"]).max()
    print(f"{what}: the final state from the model by {gap:.3g}, tolerance {tol['state']:.3g}")
    assert gap <= tol["state"]


def optimize(lm, n_max, f_min_dx_norm):
    ok, scalars, trace = lm.Optimize(n_max, f_min_dx_norm, L.TAU, 0.0, 10)
    return dict(ok=ok, scalars=scalars, trace=trace, state=lm.state.cpu().numpy())


def model_pair(kind, spec, **kw):
    """The model's Optimize(8) by Cholesky, and the tolerance from the same by LU.  No compared round may form its gain ratio
    from cancelled figures: a decision must not hang on the last digits."""
    kw = dict(kw, n_max_iterations=8, n_extra_on_reject=10, stop_when_done=True)
    chol = R.run_robust(kind, 18, spec, **kw)
    assert np.abs(chol["trace"][:L.compared_rounds(chol), L.T_RHO]).min() >= 0.02    # (the floor of tests/test_lm_model_host.py)
    return chol, R.tolerance(chol, R.run_robust(kind, 18, spec, solver="lu", **kw))


def test_reference_loop_on_the_outlier_graph():
    """tests/golden/robust/se3_outliers.npz: the reference's LM on the SE(3) fixture with eight wrong measurements, CEdgePose3D
    weighting them by Huber(|err| / 0.3).  Optimize(n_max) for n_max = 1 .. 8 with the reference's anchor: the weights after
    Begin are the reference's own, decisions and counters are the model's (which are the reference's: its iteration counts),
    the figures within the tolerance, chi^2 and the state no further from the reference's than the model's are, plus that."""
    ref, runs = R.load_golden("se3_outliers"), R.outlier_runs()
    f_min = float(ref["f_min_dx_norm"])
    _, tol = model_pair("se3", R.SE3_REFERENCE, z=ref["z"], f_min_dx_norm=f_min, unary=ref["unary"])
    lm = make_lm("se3", R.SE3_REFERENCE, z=ref["z"], unary=ref["unary"])
    start = dev(lm.graph.fx["state"])
    lm.Begin(0.0, L.TAU, f_min, 8, 10)
    assert lm.Sync()[0]
    w = device_view(lm.graph.asm.Robust_Weights_ptr(), lm.graph.n_edges).cpu().numpy()
    print("the weights after Begin from the reference's by", np.abs(w - ref["weights"]).max())
    assert np.array_equal(w == 1, ref["weights"] == 1) and np.all(np.abs(w - ref["weights"]) <= TOL * ref["weights"])
    scale = np.abs(ref["states"]).max()
    for n_max, model in enumerate(runs, 1):
        lm.state.copy_(start)
        run = optimize(lm, n_max, f_min)
        compare_with_model(f"se3_outliers Optimize({n_max})", run, model, tol)
        assert run["scalars"][L.N_ROUNDS] == ref["n_iterations"][n_max - 1]
        chi2_ref, state_ref = float(ref["chi2"][n_max - 1]), ref["states"][n_max - 1]
        gap_chi2 = abs(run["scalars"][L.LAST_ERROR] - chi2_ref) / chi2_ref
        model_chi2 = abs(model["scalars"][L.LAST_ERROR] - chi2_ref) / chi2_ref
        gap_state, model_state = np.abs(run["state"] - state_ref).max() / scale, np.abs(model["state"] - state_ref).max() / scale
        print(f"se3_outliers Optimize({n_max}): from the reference: chi2 {gap_chi2:.2e} (the model {model_chi2:.2e}), "
              f"state {gap_state:.2e} (the model {model_state:.2e})")
        assert gap_chi2 <= model_chi2 + tol["chi2"] and gap_state <= model_state + tol["state"]
    assert runs[7]["scalars"][L.N_REJECTED] > 0 and runs[7]["scalars"][L.N_ACCEPTED] > 0


@pytest.mark.parametrize("name", ["huber", "cauchy"])
def test_loss_loop_on_the_outlier_graph(name):
    """A robust cost minimised: MAHALANOBIS, the set scaled by sqrt(w), the loop comparing sum 2 scale^2 rho(s)."""
    kernel = R.KERNELS[name]
    spec = R.Spec(kernel, R.MAHALANOBIS, R.LOSS, 1.0, R.DEFAULT_PARAM[kernel])
    ref = R.load_golden("se3_outliers")
    model, tol = model_pair("se3", spec, z=ref["z"])
    assert np.sum(model["start_weights"] < 0.5) >= 5
    lm = make_lm("se3", spec, z=ref["z"])
    compare_with_model(f"se3_outliers LOSS {name}", optimize(lm, 8, 0.0), model, tol)


def test_loss_loop_of_inliers_is_the_plain_loop():
    """The SE(3) fixture as it is, Huber with a scale no edge passes: every w = 1, the cost is chi^2, and the trace is the plain
    loop's within the tolerance of tests/test_lm_gpu.py."""
    plain, tol = T.device_run("se3"), L.tolerance("se3")
    lm = make_lm("se3", R.Spec(R.HUBER, R.MAHALANOBIS, R.LOSS, 1e3, 1.345))
    lm.Begin(0.0, L.TAU, 0.0)
    lm.Iterate(L.LOOPS["se3"][0])
    ok, scalars, trace = lm.Sync()
    assert ok and trace.shape == plain["trace"].shape
    for col in (L.T_ACCEPTED, L.T_STATUS, L.T_NU):
        assert np.array_equal(trace[:, col], plain["trace"][:, col])
    for q, col in (("alpha", L.T_ALPHA), ("chi2", L.T_ERROR), ("rho", L.T_RHO), ("dx_norm", L.T_DX_NORM)):
        gap = np.abs(trace[:, col] - plain["trace"][:, col]) / np.abs(plain["trace"][:, col])
        assert np.all(gap <= tol[q]), (q, gap)
    assert np.abs(lm.state.cpu().numpy() - plain["state"]).max() <= tol["state"] * np.abs(plain["state"]).max()
    assert bool((device_view(lm.graph.asm.Robust_Weights_ptr(), lm.graph.n_edges) == 1).all())


@pytest.mark.parametrize("mode", [R.REFERENCE, R.LOSS])
@pytest.mark.parametrize("solver_class", [CLinearSolver_Schur_HIP, CLinearSolver_HIP])
def test_ba_loop_with_a_robust_set(solver_class, mode):
    """The BA fixture, its one set with Huber on the Mahalanobis distance at a scale that weights half of the edges down."""
    spec = R.Spec(R.HUBER, R.MAHALANOBIS, mode, 0.5, 1.345)
    model, tol = model_pair("ba", spec, f_min_dx_norm=1e-6)
    assert np.sum(model["start_weights"] < 0.9) >= 20
    lm = make_lm("ba", spec, solver_class=solver_class)
    compare_with_model(f"ba mode {mode}", optimize(lm, 8, 1e-6), model, tol)


@pytest.mark.parametrize("mode", [R.REFERENCE, R.LOSS])
def test_a_robust_and_a_plain_set(mode):
    """The outlier graph in two sets of one Lambda: the first 30 edges robust, the other 25 plain (among them outliers that
    stay unweighted)."""
    spec = R.Spec(R.HUBER, R.MAHALANOBIS, mode, 1.0, 1.345)
    ref = R.load_golden("se3_outliers")
    mask = np.arange(55) < 30
    model, tol = model_pair("se3", spec, z=ref["z"], mask=mask)
    lm = make_lm("se3", spec, z=ref["z"], robust_edges=30)
    compare_with_model(f"two sets, mode {mode}", optimize(lm, 8, 0.0), model, tol)
    assert lm.assemblies[1].Robust_Weights_ptr() == 0 and lm.assemblies[0].Robust_Weights_ptr() != 0


@pytest.mark.parametrize("mode", [R.REFERENCE, R.LOSS])
def test_guarantees_of_the_loop(mode):
    """Round by round on the outlier graph: a rejected round leaves the state's bits; one round at a time gives the bits of all
    at once; after the status left 0 further rounds leave state, scalars and trace, and write the final state's weights over and over.  REFERENCE:
    Optimize(4), seven solves of which three are rejected; LOSS (Tukey): Optimize(3) with one extra iteration, two accepted and
    two rejected, the least |rho| 0.027."""
    spec, n_max, n_extra = (R.SE3_REFERENCE, 4, 10) if mode == R.REFERENCE else (R.Spec(R.TUKEY, R.MAHALANOBIS, R.LOSS, 1.0, 4.685), 3, 1)
    ref = R.load_golden("se3_outliers")
    whole = make_lm("se3", spec, z=ref["z"], unary=ref["unary"])
    ok, scalars, trace = whole.Optimize(n_max, 0.0, L.TAU, 0.0, n_extra)
    run = dict(ok=ok, scalars=scalars, trace=trace, state=whole.state.cpu().numpy())
    n_rounds = int(run["scalars"][L.N_ROUNDS])
    lm = make_lm("se3", spec, z=ref["z"], unary=ref["unary"])
    lm.Begin(0.0, L.TAU, 0.0, n_max, n_extra)
    states = [lm.state.clone()]
    for _ in range(n_rounds):
        lm.Iterate(1)
        ok, scalars, trace = lm.Sync()
        assert ok
        states.append(lm.state.clone())
    rest = [c for c in range(L.SCALARS) if c != L.ACCEPTED]    # (the rounds Optimize enqueued behind the last decision cleared ACCEPTED)
    assert scalars[L.STATUS] == L.BUDGET and np.array_equal(scalars[rest], run["scalars"][rest]) and np.array_equal(trace, run["trace"])
    assert scalars[L.ACCEPTED] == trace[-1, L.T_ACCEPTED] and run["scalars"][L.ACCEPTED] == 0
    assert np.array_equal(states[-1].cpu().numpy(), run["state"])
    accepted = trace[:, L.T_ACCEPTED]
    assert accepted.min() == 0 and accepted.max() == 1
    for k in range(n_rounds):
        assert torch.equal(states[k + 1], states[k]) == (accepted[k] == 0), k
    weights, trace_all = device_view(lm.graph.asm.Robust_Weights_ptr(), lm.graph.n_edges), lm.trace_dev.clone()
    lm.Iterate(1)                                          # (the handle's weights are scratch, as J0, J1 and err are: those of the
    assert lm.Sync()[0]                                    # state the last step left, from the first round behind it on)
    final_weights = weights.clone()
    lm.Iterate(2)
    ok, scalars_after, trace_after = lm.Sync()
    assert ok and torch.equal(lm.state, states[-1]) and torch.equal(lm.trace_dev, trace_all) and torch.equal(weights, final_weights)
    assert bool((final_weights < 1).any())
    assert np.array_equal(scalars_after[rest], scalars[rest]) and scalars_after[L.ACCEPTED] == 0 and np.array_equal(trace_after, trace)


def test_set_and_unset_leaves_the_plain_loop_its_bits():
    """No specification: the loop's bits before and after Set_Robust(spec), Set_Robust(None) on its handle."""
    plain = T.device_run("se3")
    lm = T.make_lm("se3")
    set_robust(lm.graph.asm, R.SE3_REFERENCE)
    assert lm.graph.asm.Robust_Weights_ptr() != 0
    lm.graph.asm.Set_Robust(None)
    assert lm.graph.asm.Robust_Weights_ptr() == 0
    lm.graph.asm.Set_Robust(None)                          # (twice is as good as once)
    lm.Begin(0.0, L.TAU, 0.0)
    lm.Iterate(L.LOOPS["se3"][0])
    ok, scalars, trace = lm.Sync()
    assert ok and np.array_equal(scalars, plain["scalars"]) and np.array_equal(trace, plain["trace"])
    assert np.array_equal(lm.state.cpu().numpy(), plain["state"])


# ---- refusals ----

def test_refusals():
    lm = T.make_lm("se3")
    g, lib, s = lm.graph, lm._lib, lm._solver
    a = g.asm._a
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    q = buf.data_ptr()

    def refused(rc, msg, solver=s):
        assert (rc, solver._error()) == (ERR_INVALID, msg)

    def spec(kernel=R.HUBER, basis=R.MAHALANOBIS, mode=R.REFERENCE, scale=1.0, param=1.345):
        return C.byref(H.Robust(kernel, basis, mode, scale, param))
    out = C.c_void_p(1)
    # null handles: nowhere to leave a text
    assert lib.slampp_hip_assembly_set_robust(None, spec()) == ERR_INVALID
    assert lib.slampp_hip_assembly_robust_weights(None, C.byref(out)) == ERR_INVALID and out.value is None
    assert lib.slampp_hip_robust_weights_device_async(None, q, q, q) == ERR_INVALID
    assert lib.slampp_hip_robust_scale_device_async(None, q, q, q, q) == ERR_INVALID
    assert lib.slampp_hip_robust_chi_squared_device_async(None, q, q, q) == ERR_INVALID
    refused(lib.slampp_hip_assembly_robust_weights(a, None), "robust: null pointer")
    # no specification
    none = "robust: no robust kernel is set on this assembly"
    refused(lib.slampp_hip_robust_weights_device_async(a, q, q, q), none)
    refused(lib.slampp_hip_robust_scale_device_async(a, q, q, q, q), none)
    refused(lib.slampp_hip_robust_chi_squared_device_async(a, q, q, q), none)
    # the specification
    for kernel in (0, 5, -1):
        refused(lib.slampp_hip_assembly_set_robust(a, spec(kernel=kernel)), "robust: unknown kernel")
    for basis in (0, 4):
        refused(lib.slampp_hip_assembly_set_robust(a, spec(basis=basis)), "robust: unknown basis")
    for mode in (0, 3):
        refused(lib.slampp_hip_assembly_set_robust(a, spec(mode=mode)), "robust: unknown mode")
    for bad in (0.0, -1.0, float("nan")):
        refused(lib.slampp_hip_assembly_set_robust(a, spec(scale=bad)), "robust: the scale and the parameter must be positive")
        refused(lib.slampp_hip_assembly_set_robust(a, spec(param=bad)), "robust: the scale and the parameter must be positive")
    for basis in (R.ERROR_NORM, R.CHI2):
        refused(lib.slampp_hip_assembly_set_robust(a, spec(basis=basis, mode=R.LOSS)),
                "robust: SLAMPP_HIP_ROBUST_MODE_LOSS needs SLAMPP_HIP_ROBUST_BASIS_MAHALANOBIS")
    assert g.asm.Robust_Weights_ptr() == 0                 # (a refused specification sets nothing)
    # null pointers, with a specification
    assert lib.slampp_hip_assembly_set_robust(a, spec(basis=R.ERROR_NORM)) == 0
    refused(lib.slampp_hip_robust_weights_device_async(a, None, None, q), "robust: null pointer")
    refused(lib.slampp_hip_robust_chi_squared_device_async(a, q, q, q), "robust: the robust cost needs SLAMPP_HIP_ROBUST_BASIS_MAHALANOBIS")
    assert lib.slampp_hip_assembly_set_robust(a, spec(basis=R.CHI2)) == 0
    refused(lib.slampp_hip_robust_weights_device_async(a, None, q, q), "robust: null pointer")
    refused(lib.slampp_hip_robust_chi_squared_device_async(a, q, q, q), "robust: the robust cost needs SLAMPP_HIP_ROBUST_BASIS_MAHALANOBIS")
    assert lib.slampp_hip_assembly_set_robust(a, spec()) == 0
    for args in ((None, q, q), (q, None, q), (q, q, None)):
        refused(lib.slampp_hip_robust_scale_device_async(a, q, *args), "robust: null pointer")
        refused(lib.slampp_hip_robust_chi_squared_device_async(a, *args), "robust: null pointer")
    # the loop: a set with a specification and a weight array
    both = "lm: an edge set has both a robust kernel and a weight array"
    lm._sets[0].p_weight_dev = q
    refused(lib.slampp_hip_lm_iterate_device_async(C.byref(lm._problem), 1), both)
    refused(lib.slampp_hip_lm_begin_device_async(C.byref(lm._problem), 1.0, 0.0, 0.0, 5, 10), both)
    lm._sets[0].p_weight_dev = None
    with pytest.raises(ValueError):
        CLevenbergMarquardt_HIP(g.solver, g.lam, [dict(assembly=g.asm, edge_type=H.EDGE_SE3, measurement=g.z, sigma_inv=g.sigma_inv,
                                                       weight=np.ones(g.n_edges), robust=as_dict(R.SE3_REFERENCE))],
                                T.vertex_ranges("se3", g.fx), g.fx["state"])
    # nothing was enqueued by any of them
    assert s.sync() and not bool(buf.any())
    # an assembly that another structure has outdated
    ba = T.Graph("ba")
    s._set_structure(ba.lam)
    stale = "robust: set_structure was called after this assembly was created"
    refused(lib.slampp_hip_assembly_set_robust(a, spec()), stale)
    refused(lib.slampp_hip_assembly_set_robust(a, None), stale)
    refused(lib.slampp_hip_robust_weights_device_async(a, q, q, q), stale)
    refused(lib.slampp_hip_robust_scale_device_async(a, q, q, q, q), stale)
    refused(lib.slampp_hip_robust_chi_squared_device_async(a, q, q, q), stale)
