"""A numpy model of the robust kernels on the device (csrc/robust.hip, include/slampp_hip.h) on top of tests/linearize_model.py and
tests/lm_model.py, which it imports unchanged: the weight functions w(s) of the reference's loss functions, rho(s) with
rho' = s w(s) and rho(0) = 0, the three bases, the weighted dense system in both modes, and ``run_robust``, which is
``lm_model.run`` with these in place.  numpy's double arithmetic rounds every operation and fuses nothing: w(s) here is the
header's expression operation for operation (Welsch aside, whose exp is the library's)."""
import collections
import os

import numpy as np

import linearize_model as M
import lm_model as L

HUBER, CAUCHY, TUKEY, WELSCH = 1, 2, 3, 4
ERROR_NORM, CHI2, MAHALANOBIS = 1, 2, 3
REFERENCE, LOSS = 1, 2
KERNELS = {"huber": HUBER, "cauchy": CAUCHY, "tukey": TUKEY, "welsch": WELSCH}
BASES = {"error_norm": ERROR_NORM, "chi2": CHI2, "mahalanobis": MAHALANOBIS}
DEFAULT_PARAM = {HUBER: 1.345, CAUCHY: 2.385, TUKEY: 4.685, WELSCH: 2.985}

Spec = collections.namedtuple("Spec", "kernel basis mode scale param")
SE3_REFERENCE = Spec(HUBER, ERROR_NORM, REFERENCE, 0.3, 1.345)   # CEdgePose3D: SE3_Types.h:128-129


def weight(kernel, a, s):
    """w(s), RobustLoss.h:103, :153, :206, :433, elementwise on an array of s >= 0."""
    s = np.asarray(s, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        if kernel == HUBER:
            return np.where(s <= a, 1.0, a / s)
        if kernel == CAUCHY:
            return a * a / (a * a + s * s)
        if kernel == TUKEY:
            return np.where(s <= a, (1 - (s * s) / (a * a)) * (1 - (s * s) / (a * a)), 0.0)
        if kernel == WELSCH:
            return np.exp(-s * s / (a * a))
    raise ValueError("unknown kernel")


def rho(kernel, a, s):
    s = np.asarray(s, dtype=np.float64)
    with np.errstate(under="ignore", over="ignore"):
        if kernel == HUBER:
            return np.where(s <= a, s * s / 2, a * (s - a / 2))
        if kernel == CAUCHY:
            return (a * a / 2) * np.log1p(s * s / (a * a))
        if kernel == TUKEY:
            t = 1 - (s * s) / (a * a)
            return np.where(s <= a, (a * a / 6) * (1 - t * t * t), a * a / 6)
        if kernel == WELSCH:
            return (a * a / 2) * -np.expm1(-s * s / (a * a))
    raise ValueError("unknown kernel")


def quadratic_form(err, sigma_inv):
    return np.einsum("ei,eij,ej->e", err, sigma_inv, err)


def basis_argument(basis, scale, err, sigma_inv=None):
    """s of every edge: err [E, rd], sigma_inv [E, rd, rd] (not read with ERROR_NORM)."""
    if basis == ERROR_NORM:
        return np.sqrt(np.einsum("ei,ei->e", err, err)) / scale
    q = quadratic_form(err, sigma_inv)
    if basis == CHI2:
        return q / scale
    if basis == MAHALANOBIS:
        return np.sqrt(q) / scale
    raise ValueError("unknown basis")


def weights(spec, err, sigma_inv=None, mask=None):
    """w of every edge; ``mask`` [E] bool: the edges of the robust set (the others are weighted 1)."""
    w = weight(spec.kernel, spec.param, basis_argument(spec.basis, spec.scale, err, sigma_inv))
    return w if mask is None else np.where(mask, w, 1.0)


def cost_terms(spec, err, sigma_inv, mask=None):
    """What the loop compares, per edge: err^T Omega err (REFERENCE: f_Chi_Squared_Error does not weight, SE3_Types.h:323-331),
    2 scale^2 rho(s) of the MAHALANOBIS s (LOSS)."""
    q = quadratic_form(err, sigma_inv)
    if spec.mode == REFERENCE:
        return q
    assert spec.basis == MAHALANOBIS
    r = 2 * (spec.scale * spec.scale) * rho(spec.kernel, spec.param, np.sqrt(q) / spec.scale)
    return r if mask is None else np.where(mask, r, q)


def cost(spec, err, sigma_inv, mask=None):
    return float(np.sum(cost_terms(spec, err, sigma_inv, mask)))


def scaled(w, *arrays):
    """Each array [E, ...] times sqrt(w) of its edge (slampp_hip_robust_scale_device_async)."""
    r = np.sqrt(w)
    return [a * r.reshape((-1,) + (1,) * (a.ndim - 1)) for a in arrays]


def dense_system(spec, w, cumsum, v0, v1, J0, J1, sigma_inv, err, unary=None):
    """Lambda and eta with the weights in place.  REFERENCE: every block of Lambda times w, vertex 1's eta times w and
    vertex 0's times w^2 (BaseTypes_Binary.h:813-815, :821 against :834, :843).  LOSS: the plain system of the scaled set."""
    args = () if unary is None else unary
    if spec.mode == LOSS:
        J0s, J1s, errs = scaled(w, J0, J1, err)
        return M.dense_system(cumsum, v0, v1, J0s, J1s, sigma_inv, errs, *args)
    n = int(cumsum[-1])
    lam, eta = M.dense_system(cumsum, v0, v1, J0, J1, sigma_inv * w[:, None, None], err, *args)
    for e in range(len(v0)):                             # the second w on vertex 0's right-hand side
        s = slice(cumsum[v0[e]], cumsum[v0[e] + 1])
        eta[s] += (w[e] * w[e] - w[e]) * (J0[e].T @ sigma_inv[e] @ err[e])
    assert lam.shape == (n, n)
    return lam, eta


def initial_damping(spec, w, J0, J1, sigma_inv):
    if spec.mode == LOSS:
        J0, J1 = scaled(w, J0, J1)
        return L.initial_damping(J0, J1, sigma_inv)
    return L.initial_damping(J0, J1, sigma_inv, w)


def run_robust(kind, n_rounds, spec, z=None, mask=None, f_alpha=0.0, f_tau=L.TAU, f_min_dx_norm=0.0, n_max_iterations=1 << 30,
               n_extra_on_reject=10, state=None, unary="default", stop_when_done=False, solver="chol"):
    """``lm_model.run`` on a fixture with measurements ``z`` (None: the fixture's) and the robust kernel ``spec`` on
    the edges of ``mask`` (None: all).  The result of ``lm_model.run``, and ``start_weights``: w at the start state."""
    fx = M.load_fixture(kind)
    cs, v0, v1, S, P = fx["cumsum"], fx["v0"], fx["v1"], fx["sigma_inv"], fx["params"]
    z = fx["z"] if z is None else z
    kinds = M.vertex_kinds(kind, fx)
    if isinstance(unary, str):
        unary = L.unary_of(kind, fx)
    state = np.array(fx["state"] if state is None else state, dtype=np.float64)
    n = len(state)
    _, err, J0, J1 = M.linearize(kind, state, cs, v0, v1, z, P)
    start_weights = weights(spec, err, S, mask)
    alpha = f_tau * initial_damping(spec, start_weights, J0, J1, S) if f_tau > 0 else f_alpha
    s = L.begin(alpha, cost(spec, err, S, mask), f_min_dx_norm, n_max_iterations, n_extra_on_reject)
    trace = np.zeros((n_rounds, L.RECORD))
    states, scalars_after = [state.copy()], []
    for _ in range(n_rounds):
        if stop_when_done and s[L.STATUS] != 0:
            break
        _, err, J0, J1 = M.linearize(kind, state, cs, v0, v1, z, P)
        lam, eta = dense_system(spec, weights(spec, err, S, mask), cs, v0, v1, J0, J1, S, err, unary)
        flag, dx = False, np.full(n, np.nan)
        if solver == "chol":
            try:
                C = np.linalg.cholesky(lam + s[L.ALPHA] * np.eye(n))
                dx = np.linalg.solve(C.T, np.linalg.solve(C, eta))
            except np.linalg.LinAlgError:
                flag = True
        else:
            dx = np.linalg.solve(lam + s[L.ALPHA] * np.eye(n), eta)
        if s[L.STATUS] == 0:
            s[L.DX_DX], s[L.DX_ETA] = float(dx @ dx), float(dx @ eta)
        trial = M.state_plus(kinds, state, cs, np.nan_to_num(dx))
        _, err_trial, _, _ = M.linearize(kind, trial, cs, v0, v1, z, P)
        L.decide(s, flag, [cost(spec, err_trial, S, mask)], trace)
        if s[L.ACCEPTED]:
            state = trial
        states.append(state.copy())
        scalars_after.append(s.copy())
    return {"state": state, "scalars": s, "trace": trace[:int(s[L.N_RECORDS])], "states": np.array(states),
            "scalars_after": np.array(scalars_after), "start_weights": start_weights}


_cache = {}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "robust")


def load_golden(name):
    """tests/golden/robust/<name>.npz as a dict (tests/golden/make_robust_golden.py says what it holds); se3_outliers with
    ``unary``, the anchor of the reference's system in the form ``run_robust`` takes."""
    if name not in _cache:
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        g = {k: z[k] for k in z.files}
        if "unary_factor" in g:
            error = g["unary_error"] if np.any(g["unary_error"]) else None
            g["unary"] = (int(g["unary_vertex"]), g["unary_factor"], error)
        _cache[name] = g
    return _cache[name]


OUTLIER_SEED = 20   # (with 7 the reference rejects no step; of 8 .. 39 this one leaves the widest margin in |rho|, 0.256)


def outlier_measurements(seed=OUTLIER_SEED):
    """The recipe of se3_outliers: the SE(3) fixture's measurements with edges 3, 10, .. 52 perturbed -- the translation by
    N(0, 0.8), the rotation by N(0, 0.3)."""
    z = M.load_fixture("se3")["z"].copy()
    rng = np.random.default_rng(seed)
    for e in np.arange(3, 55, 7):
        z[e, :3] += rng.normal(0, 0.8, 3)
        z[e, 3:] += rng.normal(0, 0.3, 3)
    return z


def outlier_runs():
    """The model's Optimize(n_max, f_min_dx_norm) for n_max = 1 .. 8 on se3_outliers with the reference's kernel and anchor,
    computed once per process and shared (do not write into them)."""
    if "runs" not in _cache:
        g = load_golden("se3_outliers")
        _cache["runs"] = [run_robust("se3", n_max + 10, SE3_REFERENCE, z=g["z"], f_min_dx_norm=float(g["f_min_dx_norm"]),
                                     n_max_iterations=n_max, n_extra_on_reject=10, unary=g["unary"], stop_when_done=True)
                          for n_max in range(1, 9)]
    return _cache["runs"]


def tolerance(chol, lu):
    """``lm_model.tolerance`` for a loop of ``run_robust``: per quantity 100 x what solving by Cholesky (``chol``) or by LU
    (``lu``, the same call with ``solver="lu"``) moves it over the compared rounds, and not below the project's 1e-10."""
    k = L.compared_rounds(chol)
    assert L.compared_rounds(lu) == k and len(lu["trace"]) == len(chol["trace"])
    ta, tb = chol["trace"][:k], lu["trace"][:k]
    out = {q: float((np.abs(ta[:, c] - tb[:, c]) / np.abs(ta[:, c])).max()) for q, c in L._COLUMN.items()}
    out["state"] = float(np.abs(chol["state"] - lu["state"]).max() / np.abs(chol["state"]).max())
    return {q: max(1e-10, 100 * v) for q, v in out.items()}
