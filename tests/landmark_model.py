"""An exact model of the pose-landmark and stereo edges of slampp_hip_linearize_device_async (SLAMPP_HIP_EDGE_POSE_LANDMARK_2D,
_POSE_LANDMARK_3D, _P2SC_XYZ) in torch fp64 on the CPU, in the manner of tests/linearize_model.py, whose helpers it uses, and of
graphs with several edge sets: ``linearize``, ``dense_system`` and ``run`` (the LM loop of tests/lm_model.py over a list of sets).

The 3D and the stereo Jacobians are autograd of eps -> h(x (+) eps, .) at eps = 0.  The 2D ones are the reference's closed
form with its range clamp (2DSolverBase.h:475-495), evaluated in numpy in the order of the C code -- autograd is NaN at r = 0
and knows nothing of the clamp; ``lm2d_jacobians_autograd`` is there to check the closed form on the regular edges.

A fixture (tests/golden/landmark/<name>.npz, tests/golden/make_landmark_golden.py) holds one graph: the landmark or stereo set
as ``v0, v1, z, sigma_inv`` (vertex 0 the pose or camera) with the reference's outputs, and for lm2d and lm3d the pose-pose set
as ``a_v0, a_v1, a_z, a_sigma_inv``."""
import os

import numpy as np
import torch

import linearize_model as M
import lm_model as LM

F64 = torch.float64
NAMES = ("lm2d", "lm3d", "stereo")
EDGE_SHAPES = dict(M.EDGE_SHAPES, lm2d=(3, 2, 2), lm3d=(6, 3, 3), stereo=(6, 3, 3))   # d0, d1, rd
POSE_KIND = {"lm2d": "se2", "lm3d": "se3", "stereo": "se3"}                           # the vertex type of vertex 0
MIN_RANGE = 1e-5


# ---- pose-landmark 2D ----

def lm2d_expectation(x0, x1, clamp=True):
    d = x1 - x0[:, :2]
    r = torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    b = M.clamp_angle_2pi(torch.atan2(d[:, 1], d[:, 0]) - x0[:, 2])
    if clamp:
        r = torch.where(r.abs() < MIN_RANGE, torch.full_like(r, MIN_RANGE), r)
    return torch.stack([r, b], -1)


def lm2d_error(z, h):
    e = z - h
    return torch.stack([e[:, 0], M.clamp_angular_error_2pi(e[:, 1])], -1)


def lm2d_jacobians(x0, x1):
    """The closed form, operation for operation as 2DSolverBase.h:482-495 (numpy: IEEE doubles, nothing fused)."""
    x0, x1 = np.asarray(x0), np.asarray(x1)
    de, dn = x1[:, 0] - x0[:, 0], x1[:, 1] - x0[:, 1]
    r = np.sqrt(de * de + dn * dn)
    r = np.where(np.abs(r) < MIN_RANGE, MIN_RANGE, r)
    r2, o = r * r, np.zeros_like(r)
    J0 = np.stack([np.stack([-de / r, -dn / r, o], -1), np.stack([dn / r2, -de / r2, o - 1], -1)], 1)
    J1 = np.stack([np.stack([de / r, dn / r], -1), np.stack([-dn / r2, de / r2], -1)], 1)
    return J0, J1


def lm2d_jacobians_autograd(x0, x1):
    E = x0.shape[0]
    return (M._batched_jacobian(lambda e: lm2d_expectation(x0 + e, x1, clamp=False), E, 3),
            M._batched_jacobian(lambda e: lm2d_expectation(x0, x1 + e, clamp=False), E, 2))


# ---- pose-landmark 3D: h = R0^T (X - t0) ----

def _lm3d_h(t0, R0, X):
    return M._mv(R0.transpose(-1, -2), X - t0)


def lm3d_expectation(x0, x1):
    return _lm3d_h(x0[:, :3], M.so3_exp(x0[:, 3:]), x1)


def lm3d_jacobians(x0, x1):
    E = x0.shape[0]
    t0, R0 = x0[:, :3], M.so3_exp(x0[:, 3:])
    return (M._batched_jacobian(lambda e: _lm3d_h(*M._se3_plus_tR(t0, R0, e), x1), E, 6),
            M._batched_jacobian(lambda e: _lm3d_h(t0, R0, x1 + e), E, 3))


# ---- stereo: K = (fx, fy, cx, cy, k, baseline) per edge; the radial term is linear in |p| (BASolverBase.h:516-517) ----

def _radial(p, k):
    return (1 + k * torch.sqrt((p * p).sum(-1)))[:, None] * p


def _project_stereo(t, R, X, K):
    x = M._mv(R, X) + t
    k = K[:, 4] / (0.5 * (K[:, 0] + K[:, 1]))
    py = K[:, 1] * x[:, 1] / x[:, 2]
    left = K[:, 2:4] + _radial(torch.stack([K[:, 0] * x[:, 0] / x[:, 2], py], -1), k)
    right = K[:, 2:4] + _radial(torch.stack([K[:, 0] * (x[:, 0] - K[:, 5]) / x[:, 2], py], -1), k)
    return torch.cat([left, right[:, :1]], -1)


def stereo_expectation(cam, X, K):
    return _project_stereo(cam[:, :3], M.so3_exp(cam[:, 3:]), X, K)


def stereo_jacobians(cam, X, K):
    E = cam.shape[0]
    t, R = cam[:, :3], M.so3_exp(cam[:, 3:])
    return (M._batched_jacobian(lambda e: _project_stereo(*M._se3_plus_tR(t, R, e), X, K), E, 6),
            M._batched_jacobian(lambda e: _project_stereo(t, R, X + e, K), E, 3))


# ---- whole edge sets on numpy arrays, in the layout of the C ABI ----

def linearize(kind, state, cumsum, v0, v1, measurement, params=None):
    """As ``linearize_model.linearize``, for its kinds and for "lm2d", "lm3d" and "stereo" (``params``: six per block column)."""
    if kind in M.EDGE_SHAPES:
        return M.linearize(kind, state, cumsum, v0, v1, measurement, params)
    d0, d1, _ = EDGE_SHAPES[kind]
    state, z = M._t(state), M._t(measurement)
    o0, o1 = np.asarray(cumsum)[np.asarray(v0)], np.asarray(cumsum)[np.asarray(v1)]
    x0 = torch.stack([state[o:o + d0] for o in o0])
    x1 = torch.stack([state[o:o + d1] for o in o1])
    if kind == "lm2d":
        h = lm2d_expectation(x0, x1)
        J0, J1 = lm2d_jacobians(x0.numpy(), x1.numpy())
        return h.numpy(), lm2d_error(z, h).numpy(), J0, J1
    if kind == "lm3d":
        h, (J0, J1) = lm3d_expectation(x0, x1), lm3d_jacobians(x0, x1)
    else:
        K = M._t(params).reshape(-1, 6)[np.asarray(v0)]
        h, (J0, J1) = stereo_expectation(x0, x1, K), stereo_jacobians(x0, x1, K)
    return h.numpy(), (z - h).numpy(), J0.numpy(), J1.numpy()


_cache = {}


def load_fixture(name):
    if ("fixture", name) not in _cache:
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "landmark", name + ".npz"))
        fx = {k: z[k] for k in z.files}
        for k in ("cumsum", "v0", "v1", "a_v0", "a_v1"):
            if k in fx:
                fx[k] = fx[k].astype(np.int64)
        fx["params"] = fx["params"] if fx["params"].size else None
        _cache["fixture", name] = fx
    return _cache["fixture", name]


def fixture_model(name):
    """The model on a fixture's landmark or stereo set (all of it), computed once and shared: (h, err, J0, J1)."""
    if ("model", name) not in _cache:
        fx = load_fixture(name)
        _cache["model", name] = linearize(name, fx["state"], fx["cumsum"], fx["v0"], fx["v1"], fx["z"], fx["params"])
    return _cache["model", name]


def write_driver_input(path, name, fx):
    """The input file of tests/landmark_golden_driver.cpp and tests/landmark_math_driver.cpp."""
    with open(path, "wb") as f:
        np.array([5 + NAMES.index(name), len(fx["cumsum"]) - 1, len(fx["v0"]), int(fx["n_first_pose"]), int(fx["n_poses"])], np.int64).tofile(f)
        params = np.zeros(0) if fx["params"] is None else fx["params"]
        for a in (fx["state"], fx["v0"], fx["v1"], fx["z"], np.transpose(fx["sigma_inv"], (0, 2, 1)), params, fx["dx"]):
            np.ascontiguousarray(a).tofile(f)


def vertex_kinds(name, fx):
    first, n_poses = int(fx["n_first_pose"]), int(fx["n_poses"])
    return [POSE_KIND[name] if first <= v < first + n_poses else "euclidean" for v in range(len(fx["cumsum"]) - 1)]


def vertex_ranges(name, fx):
    """(vertex kind, first, last) runs covering the block columns."""
    kinds, out = vertex_kinds(name, fx), []
    for v, k in enumerate(kinds):
        if out and out[-1][0] == k:
            out[-1][2] = v + 1
        else:
            out.append([k, v, v + 1])
    return [tuple(r) for r in out]


def edge_sets(name, regular_only=True):
    """The fixture's edge sets in the order the tests assemble them: dicts of ``kind, v0, v1, z, sigma_inv, params``.  The
    loops leave the close edges of lm2d out (``regular_only``)."""
    fx = load_fixture(name)
    n = int(fx["n_regular"]) if regular_only else len(fx["v0"])
    sets = []
    if "a_v0" in fx:
        sets.append(dict(kind=POSE_KIND[name], v0=fx["a_v0"], v1=fx["a_v1"], z=fx["a_z"], sigma_inv=fx["a_sigma_inv"], params=None))
    sets.append(dict(kind=name, v0=fx["v0"][:n], v1=fx["v1"][:n], z=fx["z"][:n], sigma_inv=fx["sigma_inv"][:n], params=fx["params"]))
    return sets


def linearize_sets(sets, state, cumsum):
    return [linearize(s["kind"], state, cumsum, s["v0"], s["v1"], s["z"], s["params"]) for s in sets]


def dense_system(cumsum, sets, lins, unary_vertex=None, unary_factor=None, unary_error=None, weights=None):
    """Lambda and eta of every set added up (``lins``: what ``linearize_sets`` gave), the unary factor once."""
    n = int(cumsum[-1])
    lam, eta = np.zeros((n, n)), np.zeros(n)
    for i, (s, (_, err, J0, J1)) in enumerate(zip(sets, lins)):
        S = s["sigma_inv"] if weights is None or weights[i] is None else s["sigma_inv"] * np.asarray(weights[i])[:, None, None]
        a, b = M.dense_system(cumsum, s["v0"], s["v1"], J0, J1, S, err)
        lam += a
        eta += b
    if unary_vertex is not None:
        s = slice(cumsum[unary_vertex], cumsum[unary_vertex + 1])
        lam[s, s] += unary_factor.T @ unary_factor
        if unary_error is not None:
            eta[s] += unary_error
    return lam, eta


def unary_of(name, fx):
    """The anchor of the loops: 100 I on the first pose of lm2d and lm3d, none for stereo, whose gauge the damping holds."""
    if name == "stereo":
        return None
    v = int(fx["n_first_pose"])
    return v, 100.0 * np.eye(int(fx["cumsum"][v + 1] - fx["cumsum"][v])), None


def run(name, n_rounds, f_alpha=0.0, f_tau=LM.TAU, f_min_dx_norm=0.0, n_max_iterations=1 << 30, n_extra_on_reject=10, solver="chol",
        state=None):
    """``lm_model.run`` over the edge sets of a fixture: its begin, decide and initial damping, one chi^2 part per set."""
    fx = load_fixture(name)
    cs, sets, kinds, unary = fx["cumsum"], edge_sets(name), vertex_kinds(name, fx), unary_of(name, fx)
    state = np.array(fx["state"] if state is None else state, dtype=np.float64)
    n = len(state)

    def parts(lins):
        return [M.chi2(lin[1], s["sigma_inv"]) for s, lin in zip(sets, lins)]
    lins = linearize_sets(sets, state, cs)
    alpha = f_tau * max(LM.initial_damping(lin[2], lin[3], s["sigma_inv"]) for s, lin in zip(sets, lins)) if f_tau > 0 else f_alpha
    error = 0.0
    for p in parts(lins):
        error += p
    s = LM.begin(alpha, error, f_min_dx_norm, n_max_iterations, n_extra_on_reject)
    trace = np.zeros((n_rounds, LM.RECORD))
    states, scalars_after = [state.copy()], []
    for _ in range(n_rounds):
        lins = linearize_sets(sets, state, cs)
        lam, eta = dense_system(cs, sets, lins, *(unary if unary is not None else ()))
        A = lam + s[LM.ALPHA] * np.eye(n)
        flag, dx = False, np.full(n, np.nan)
        if solver == "chol":
            try:
                L = np.linalg.cholesky(A)
                dx = np.linalg.solve(L.T, np.linalg.solve(L, eta))
            except np.linalg.LinAlgError:
                flag = True
        else:
            dx = np.linalg.solve(A, eta)
        if s[LM.STATUS] == 0:
            s[LM.DX_DX], s[LM.DX_ETA] = float(dx @ dx), float(dx @ eta)
        trial = M.state_plus(kinds, state, cs, np.nan_to_num(dx))
        LM.decide(s, flag, parts(linearize_sets(sets, trial, cs)), trace)
        if s[LM.ACCEPTED]:
            state = trial
        states.append(state.copy())
        scalars_after.append(s.copy())
    return {"state": state, "scalars": s, "trace": trace[:int(s[LM.N_RECORDS])], "states": np.array(states),
            "scalars_after": np.array(scalars_after)}


# the loops the tests compare against: (rounds, f_min_dx_norm).  Both stop on |dx|, as lm_model's BA loop does.  lm2d at 1e-4, in
# its eighth round: two rounds on its steps are of 1e-6, chi^2 moves in its 13th digit and rho is formed from cancelled
# figures -- a decision must not hang on the last digits
LOOPS = {"lm2d": (10, 1e-4), "stereo": (8, 1e-6)}


def fixture_run(name, solver="chol"):
    if ("run", name, solver) not in _cache:
        n_rounds, f_min_dx_norm = LOOPS[name]
        _cache["run", name, solver] = run(name, n_rounds, f_min_dx_norm=f_min_dx_norm, solver=solver)
    return _cache["run", name, solver]


def sensitivity(name):
    """As ``lm_model.sensitivity``: the Cholesky-versus-LU spread of this model's own loop on the fixture, per quantity."""
    if ("sensitivity", name) not in _cache:
        a, b = fixture_run(name, "chol"), fixture_run(name, "lu")
        k = min(LM.compared_rounds(a), LM.compared_rounds(b))
        ta, tb = a["trace"][:k], b["trace"][:k]
        out = {q: float((np.abs(ta[:, c] - tb[:, c]) / np.abs(ta[:, c])).max()) for q, c in LM._COLUMN.items()}
        out["state"] = float(np.abs(a["state"] - b["state"]).max() / np.abs(a["state"]).max())
        _cache["sensitivity", name] = out
    return _cache["sensitivity", name]


def tolerance(name):
    """The project's rule: max(1e-10, 100 x sensitivity) per quantity."""
    return {q: max(1e-10, 100 * v) for q, v in sensitivity(name).items()}
