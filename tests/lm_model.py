"""A model of the device-decided Levenberg-Marquardt loop (slampp_hip_lm_begin_device_async, slampp_hip_lm_iterate_device_async) in
numpy on top of tests/linearize_model.py: the reference's CLevenbergMarquardt_Baseline (NonlinearSolver_Lambda_LM.h:151-223) inside
the loop of CNonlinearSolver_Lambda_LM::Optimize (:915-1115), written in the order of the decide kernel on the same block of 16
scalars.  Lambda is dense here and the step comes from numpy (Cholesky, or LU to measure how much the way of solving matters)."""
import math

import numpy as np

import linearize_model as M

(ALPHA, NU, LAST_ERROR, ERROR, DX_DX, DX_ETA, RHO, ACCEPTED, STATUS, N_ROUNDS, N_ACCEPTED, N_REJECTED, ROUNDS_LEFT, EXTRA_LEFT,
 MIN_DX_NORM, N_RECORDS, SCALARS) = range(17)
RUNNING, CONVERGED, NOT_POSDEF, BUDGET = range(4)
T_ALPHA, T_ERROR, T_RHO, T_DX_NORM, T_ACCEPTED, T_STATUS, T_LAST_ERROR, T_NU, RECORD = range(9)
TAU = 1e-3


def begin(alpha, last_error, f_min_dx_norm, n_max_iterations, n_extra_on_reject):
    s = np.zeros(SCALARS)
    s[ALPHA], s[NU], s[LAST_ERROR], s[MIN_DX_NORM] = alpha, 2.0, last_error, f_min_dx_norm
    s[ROUNDS_LEFT], s[EXTRA_LEFT] = max(n_max_iterations, 0), max(n_extra_on_reject, 0)
    s[STATUS] = RUNNING if n_max_iterations > 0 else BUDGET
    return s


def decide(s, flag, chi_parts, trace=None):
    """One decision on the scalars ``s`` (in place); ``trace``: a list of [capacity, RECORD] array or None.  Python floats are
    IEEE doubles and nothing here is fused: the kernel's decision arithmetic, operation for operation."""
    if s[STATUS] != 0:
        s[ACCEPTED] = 0.0
        return
    error = 0.0
    for part in chi_parts:
        error += float(part)
    alpha_used, dx_dx = float(s[ALPHA]), float(s[DX_DX])
    dx_norm = math.sqrt(dx_dx) if dx_dx >= 0 else float("nan")
    alpha, nu, last, rho, accepted, status = alpha_used, float(s[NU]), float(s[LAST_ERROR]), 0.0, 0.0, RUNNING
    if flag:
        status = NOT_POSDEF
    elif dx_norm <= s[MIN_DX_NORM]:
        status = CONVERGED
    else:
        den = alpha * dx_dx + float(s[DX_ETA])
        num = last - error
        rho = num / den if den != 0 else (float("nan") if num == 0 or num != num else math.copysign(float("inf"), num) * math.copysign(1.0, den))
        if rho > 0:
            t = 2 * rho - 1
            alpha *= max(1 / 3.0, 1.0 - t * t * t)
            nu, last, accepted = 2.0, error, 1.0
            s[N_ACCEPTED] += 1
        else:
            alpha *= nu
            nu *= 2
            s[N_REJECTED] += 1
            if s[EXTRA_LEFT] > 0:
                s[EXTRA_LEFT] -= 1
                s[ROUNDS_LEFT] += 1
        s[ROUNDS_LEFT] -= 1
        if s[ROUNDS_LEFT] <= 0:
            status = BUDGET
    s[ALPHA], s[NU], s[LAST_ERROR], s[ERROR], s[RHO], s[ACCEPTED], s[STATUS] = alpha, nu, last, error, rho, accepted, status
    s[N_ROUNDS] += 1
    record = int(s[N_RECORDS])
    s[N_RECORDS] += 1
    if trace is not None and record < len(trace):
        trace[record] = (alpha_used, error, rho, dx_norm, accepted, status, last, nu)


def initial_damping(J0, J1, sigma_inv, weight=None):
    """max over the edges of the largest diagonal entry of w J0^T Omega J0 and of w J1^T Omega J1, from 0 (f_InitialDamping
    without tau); J [E, rd, d] and sigma_inv [E, rd, rd] row-major as linearize_model gives them."""
    w = np.ones(len(J0)) if weight is None else np.asarray(weight)
    m = 0.0
    for J in (J0, J1):
        if len(J):
            m = max(m, float((w[:, None] * np.einsum("erj,erc,ecj->ej", J, sigma_inv, J)).max()))
    return m


def unary_of(kind, fx):
    """The anchor the tests use: 100 I on block column 0 of the pose graphs (U^T U = 10^4 I goes onto Lambda), none for BA,
    whose gauge the damping holds."""
    if kind == "ba":
        return None
    d = int(fx["cumsum"][1] - fx["cumsum"][0])
    return 0, 100.0 * np.eye(d), None


def run(kind, n_rounds, f_alpha=0.0, f_tau=TAU, f_min_dx_norm=0.0, n_max_iterations=1 << 30, n_extra_on_reject=10, solver="chol",
        state=None, unary="default", stop_when_done=False):
    """begin + n_rounds rounds on a fixture from its own state (or ``state``); ``stop_when_done``: the rounds behind the one that
    sets the status, which change nothing, are left out.  Returns a dict: ``state``, ``scalars``, ``trace``
    [records, RECORD], ``states`` [n_rounds + 1, n] (the state before round k and after the last) and ``scalars_after`` [n_rounds,
    SCALARS]."""
    fx = M.load_fixture(kind)
    cs, v0, v1, z, S, P = fx["cumsum"], fx["v0"], fx["v1"], fx["z"], fx["sigma_inv"], fx["params"]
    kinds = M.vertex_kinds(kind, fx)
    if isinstance(unary, str):
        unary = unary_of(kind, fx)
    state = np.array(fx["state"] if state is None else state, dtype=np.float64)
    n = len(state)
    _, err, J0, J1 = M.linearize(kind, state, cs, v0, v1, z, P)
    alpha = f_tau * initial_damping(J0, J1, S) if f_tau > 0 else f_alpha
    s = begin(alpha, M.chi2(err, S), f_min_dx_norm, n_max_iterations, n_extra_on_reject)
    trace = np.zeros((n_rounds, RECORD))
    states, scalars_after = [state.copy()], []
    for _ in range(n_rounds):
        if stop_when_done and s[STATUS] != 0:
            break
        _, err, J0, J1 = M.linearize(kind, state, cs, v0, v1, z, P)
        lam, eta = M.dense_system(cs, v0, v1, J0, J1, S, err, *(unary if unary is not None else ()))
        A = lam + s[ALPHA] * np.eye(n)
        flag, dx = False, np.full(n, np.nan)
        if solver == "chol":
            try:
                L = np.linalg.cholesky(A)
                dx = np.linalg.solve(L.T, np.linalg.solve(L, eta))
            except np.linalg.LinAlgError:
                flag = True
        else:
            dx = np.linalg.solve(A, eta)
        if s[STATUS] == 0:
            s[DX_DX], s[DX_ETA] = float(dx @ dx), float(dx @ eta)
        trial = M.state_plus(kinds, state, cs, np.nan_to_num(dx))
        _, err_trial, _, _ = M.linearize(kind, trial, cs, v0, v1, z, P)
        decide(s, flag, [M.chi2(err_trial, S)], trace)
        if s[ACCEPTED]:
            state = trial
        states.append(state.copy())
        scalars_after.append(s.copy())
    return {"state": state, "scalars": s, "trace": trace[:int(s[N_RECORDS])], "states": np.array(states),
            "scalars_after": np.array(scalars_after)}


_cache = {}

# the three loops every test compares against: (kind, rounds, f_min_dx_norm)
LOOPS = {"se2": (14, 0.0), "se3": (14, 0.0), "ba": (8, 1e-6)}


def fixture_run(kind, solver="chol"):
    """The loop of LOOPS on a fixture, computed once per process and shared (do not write into it)."""
    if (kind, solver) not in _cache:
        n_rounds, f_min_dx_norm = LOOPS[kind]
        _cache[kind, solver] = run(kind, n_rounds, f_min_dx_norm=f_min_dx_norm, solver=solver)
    return _cache[kind, solver]


QUANTITIES = ("alpha", "chi2", "rho", "dx_norm", "state")
_COLUMN = {"alpha": T_ALPHA, "chi2": T_ERROR, "rho": T_RHO, "dx_norm": T_DX_NORM}


def load_reference(kind):
    """tests/golden/lm/<kind>.npz as a dict (tests/golden/make_lm_golden.py says what it holds), with ``unary`` the anchor of
    the reference's system in the form ``run`` takes."""
    import os
    if ("reference", kind) not in _cache:
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm", kind + ".npz"))
        ref = {k: z[k] for k in z.files}
        error = ref["unary_error"] if np.any(ref["unary_error"]) else None
        ref["unary"] = (int(ref["unary_vertex"]), ref["unary_factor"], error)
        _cache["reference", kind] = ref
    return _cache["reference", kind]


def reference_runs(kind):
    """The model's Optimize(n_max, f_min_dx_norm) for n_max = 1 .. 8 with the reference's anchor: a list of ``run`` results,
    computed once per process and shared."""
    if ("reference_runs", kind) not in _cache:
        ref = load_reference(kind)
        _cache["reference_runs", kind] = [run(kind, n_max + 10, f_min_dx_norm=float(ref["f_min_dx_norm"]), n_max_iterations=n_max,
                                              n_extra_on_reject=10, unary=ref["unary"], stop_when_done=True) for n_max in range(1, 9)]
    return _cache["reference_runs", kind]


def sensitivity(kind):
    """How far the Cholesky and the LU solution of the same systems carry a fixture's loop apart: the largest relative
    difference over the compared rounds of each of QUANTITIES (the state: rel-inf after the last round), as a dict.  This is
    what rounding in the linear solve alone does to the trajectory; the late SE(2) rounds, where chi^2 moves in its 12th digit,
    form rho from cancelled figures, and its sensitivity there is of order 0.1."""
    if ("sensitivity", kind) not in _cache:
        a, b = fixture_run(kind, "chol"), fixture_run(kind, "lu")
        k = compared_rounds(a)
        ta, tb = a["trace"][:k], b["trace"][:k]
        out = {q: float((np.abs(ta[:, c] - tb[:, c]) / np.abs(ta[:, c])).max()) for q, c in _COLUMN.items()}
        out["state"] = float(np.abs(a["state"] - b["state"]).max() / np.abs(a["state"]).max())
        _cache["sensitivity", kind] = out
    return _cache["sensitivity", kind]


def tolerance(kind):
    """The tolerance of a comparison with this model, per quantity: 100 x the sensitivity above, and not below the project's
    1e-10 (tests/test_linearize_gpu.py)."""
    return {q: max(1e-10, 100 * v) for q, v in sensitivity(kind).items()}


def compared_rounds(result):
    """The rounds whose figures may be compared: those that formed a gain ratio (before convergence: past it rho is 0 / 0)."""
    return int(np.sum(np.isin(result["trace"][:, T_STATUS], (RUNNING, BUDGET))))
