"""An exact model of the three edge types and the three manifold updates that slampp_hip_linearize_device_async,
slampp_hip_state_plus_device_async and slampp_hip_chi_squared_device_async compute, in torch fp64 on the CPU.

It follows the definitions of include/slampp_hip.h, not the kernels and not the reference: rotations are matrices
(``torch.linalg.matrix_exp`` of the skew matrix, the logarithm from the antisymmetric part and the trace) where the device
code uses quaternions, and the Jacobians are not written down at all: they are ``torch.autograd.functional.jacobian`` of
eps -> h(x (+) eps, .) at eps = 0.  Every function takes a batch of edges (leading dimension E); an edge's expectation
depends on its own perturbation alone, so the Jacobian of the sum over the edges with respect to all perturbations holds
every edge's Jacobian, and one call differentiates the whole batch.

Autograd yields NaN at exactly zero rotation (the derivative of |v| at 0).  The logarithm below steps around that point
with ``torch.where``, and ``se3_jacobians`` writes the closed-form limits there: Jl^-1 = Jr^-1 = I."""
import math

import numpy as np
import torch

TWO_PI = 2 * math.pi
F64 = torch.float64


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=F64)


def clamp_angle_2pi(a):
    """The angle modulo 2 pi with the sign of the angle (C's fmod)."""
    return torch.fmod(a, TWO_PI)


def clamp_angular_error_2pi(e):
    """Of a, a - 2 pi, a + 2 pi (a = e modulo 2 pi) the one of the least magnitude."""
    a = clamp_angle_2pi(e)
    b, c = a - TWO_PI, a + TWO_PI
    m = torch.where(a.abs() < b.abs(), a, b)
    return torch.where(m.abs() < c.abs(), m, c)


def skew(v):
    z = torch.zeros_like(v[..., 0])
    return torch.stack([torch.stack([z, -v[..., 2], v[..., 1]], -1), torch.stack([v[..., 2], z, -v[..., 0]], -1),
                        torch.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def so3_exp(phi):
    return torch.linalg.matrix_exp(skew(phi))


def so3_log(R):
    """The principal logarithm (angle in [0, pi))."""
    v = 0.5 * torch.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    c = 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1)
    n2 = (v * v).sum(-1)
    zero = n2 == 0
    n = torch.sqrt(torch.where(zero, torch.ones_like(n2), n2))
    k = torch.where(zero, torch.ones_like(n), torch.atan2(n, c) / n)
    return v * k[..., None]


def _mv(M, v):
    return (M @ v[..., None])[..., 0]


# ---- SE(2) ----

def se2_expectation(x0, x1):
    c, s = torch.cos(x0[:, 2]), torch.sin(x0[:, 2])
    d = x1[:, :2] - x0[:, :2]
    return torch.stack([c * d[:, 0] + s * d[:, 1], c * d[:, 1] - s * d[:, 0], clamp_angle_2pi(x1[:, 2] - x0[:, 2])], -1)


def se2_error(z, h):
    e = z - h
    return torch.cat([e[:, :2], clamp_angular_error_2pi(e[:, 2])[:, None]], -1)


def se2_plus(x, dx):
    y = x + dx
    return torch.cat([y[:, :2], clamp_angle_2pi(y[:, 2])[:, None]], -1)


# ---- SE(3): a state is (t, axis-angle); (+) is t <- t + R e_t, R <- R Exp(e_r) ----

def _se3_plus_tR(t, R, eps):
    return t + _mv(R, eps[:, :3]), R @ so3_exp(eps[:, 3:])


def _se3_h(t0, R0, t1, R1):
    R0t = R0.transpose(-1, -2)
    return torch.cat([_mv(R0t, t1 - t0), so3_log(R0t @ R1)], -1)


def se3_expectation(x0, x1):
    return _se3_h(x0[:, :3], so3_exp(x0[:, 3:]), x1[:, :3], so3_exp(x1[:, 3:]))


def se3_error(z, h):
    return torch.cat([z[:, :3] - h[:, :3], so3_log(so3_exp(z[:, 3:]) @ so3_exp(h[:, 3:]).transpose(-1, -2))], -1)


def se3_plus(x, dx):
    t, R = _se3_plus_tR(x[:, :3], so3_exp(x[:, 3:]), dx)
    return torch.cat([t, so3_log(R)], -1)


# ---- camera-point: the camera an SE(3) state, the point Euclidean; K = (fx, fy, cx, cy, k) per edge ----

def _project(t, R, X, K):
    x = _mv(R, X) + t
    p = torch.stack([K[:, 0] * x[:, 0] / x[:, 2], K[:, 1] * x[:, 1] / x[:, 2]], -1)
    k = K[:, 4] / (0.5 * (K[:, 0] + K[:, 1]))
    return K[:, 2:4] + (1 + k * (p * p).sum(-1))[:, None] * p


def p2c_expectation(cam, X, K):
    return _project(cam[:, :3], so3_exp(cam[:, 3:]), X, K)


# ---- Jacobians by autograd ----

def _batched_jacobian(f, n_edges, n_eps):
    """J[e] = d f(eps)[e] / d eps[e] at eps = 0 for f: [E, n_eps] -> [E, rd], edge e depending on eps[e] alone."""
    J = torch.autograd.functional.jacobian(lambda eps: f(eps).sum(0), torch.zeros(n_edges, n_eps, dtype=F64))   # [rd, E, n_eps]
    return J.permute(1, 0, 2).contiguous()


def se2_jacobians(x0, x1):
    E = x0.shape[0]
    return (_batched_jacobian(lambda e: se2_expectation(x0 + e, x1), E, 3),
            _batched_jacobian(lambda e: se2_expectation(x0, x1 + e), E, 3))


def se3_jacobians(x0, x1):
    E = x0.shape[0]
    t0, R0, t1, R1 = x0[:, :3], so3_exp(x0[:, 3:]), x1[:, :3], so3_exp(x1[:, 3:])
    J0 = _batched_jacobian(lambda e: _se3_h(*_se3_plus_tR(t0, R0, e), t1, R1), E, 6)
    J1 = _batched_jacobian(lambda e: _se3_h(t0, R0, *_se3_plus_tR(t1, R1, e)), E, 6)
    h = _se3_h(t0, R0, t1, R1)
    for e in torch.nonzero((h[:, 3:] == 0).all(-1)).flatten().tolist():   # exactly zero relative rotation: the limits
        J0[e, 3:, :3] = 0
        J1[e, 3:, :3] = 0
        J0[e, 3:, 3:] = -torch.eye(3, dtype=F64)
        J1[e, 3:, 3:] = torch.eye(3, dtype=F64)
    return J0, J1


def p2c_jacobians(cam, X, K):
    E = cam.shape[0]
    t, R = cam[:, :3], so3_exp(cam[:, 3:])
    return (_batched_jacobian(lambda e: _project(*_se3_plus_tR(t, R, e), X, K), E, 6),
            _batched_jacobian(lambda e: _project(t, R, X + e, K), E, 3))


# ---- whole edge sets on numpy arrays, in the layout of the C ABI ----

EDGE_SHAPES = {"se2": (3, 3, 3), "se3": (6, 6, 6), "ba": (6, 3, 2)}   # d0, d1, rd
KINDS = tuple(EDGE_SHAPES)
_cache = {}


def load_fixture(kind):
    """tests/golden/linearize/<kind>.npz as a dict of arrays (tests/golden/make_linearize_golden.py says what they are)."""
    import os
    if ("fixture", kind) not in _cache:
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linearize", kind + ".npz"))
        fx = {k: z[k] for k in z.files}
        for k in ("cumsum", "v0", "v1"):
            fx[k] = fx[k].astype(np.int64)
        fx["params"] = fx["params"] if fx["params"].size else None
        _cache["fixture", kind] = fx
    return _cache["fixture", kind]


def fixture_model(kind):
    """The model on a fixture's graph, computed once per process and shared (do not write into it): (h, err, J0, J1)."""
    if ("model", kind) not in _cache:
        fx = load_fixture(kind)
        _cache["model", kind] = linearize(kind, fx["state"], fx["cumsum"], fx["v0"], fx["v1"], fx["z"], fx["params"])
    return _cache["model", kind]


def write_driver_input(path, kind, fx):
    """The input file of tests/linearize_golden_driver.cpp and tests/linearize_math_driver.cpp."""
    with open(path, "wb") as f:
        np.array([KINDS.index(kind) + 1, len(fx["cumsum"]) - 1, len(fx["v0"]), int(fx["n_cams"])], np.int64).tofile(f)
        params = np.zeros(0) if fx["params"] is None else fx["params"]
        for a in (fx["state"], fx["v0"], fx["v1"], fx["z"], np.transpose(fx["sigma_inv"], (0, 2, 1)), params, fx["dx"]):
            np.ascontiguousarray(a).tofile(f)


def vertex_kinds(kind, fx):
    n = len(fx["cumsum"]) - 1
    if kind == "ba":
        return ["se3"] * int(fx["n_cams"]) + ["euclidean"] * (n - int(fx["n_cams"]))
    return [kind] * n


def linearize(kind, state, cumsum, v0, v1, measurement, params=None):
    """(expectation [E, rd], err [E, rd], J0 [E, rd, d0], J1 [E, rd, d1]) as numpy arrays (row-major matrices: the C ABI's
    column-major rd x d block of edge e is ``J[e].T.ravel()``)."""
    d0, d1, _ = EDGE_SHAPES[kind]
    state, z = _t(state), _t(measurement)
    o0, o1 = np.asarray(cumsum)[np.asarray(v0)], np.asarray(cumsum)[np.asarray(v1)]
    x0 = torch.stack([state[o:o + d0] for o in o0])
    x1 = torch.stack([state[o:o + d1] for o in o1])
    if kind == "se2":
        h = se2_expectation(x0, x1)
        err, (J0, J1) = se2_error(z, h), se2_jacobians(x0, x1)
    elif kind == "se3":
        h = se3_expectation(x0, x1)
        err, (J0, J1) = se3_error(z, h), se3_jacobians(x0, x1)
    else:
        K = _t(params).reshape(-1, 5)[np.asarray(v0)]
        h = p2c_expectation(x0, x1, K)
        err, (J0, J1) = z - h, p2c_jacobians(x0, x1, K)
    return h.numpy(), err.numpy(), J0.numpy(), J1.numpy()


def chi2(err, sigma_inv, weight=None):
    """sum_e w_e err_e^T Omega_e err_e; sigma_inv [E, rd, rd] (symmetric or not: row-major as given)."""
    q = np.einsum("ei,eij,ej->e", err, sigma_inv, err)
    return float(np.sum(q if weight is None else np.asarray(weight) * q))


def state_plus(kinds, state, cumsum, dx, scale=1.0):
    """The whole state moved by scale * dx; ``kinds[v]`` in {"euclidean", "se2", "se3"} per block column."""
    state, dx = _t(state), scale * _t(dx)
    out = state.clone()
    for kind, fn in (("se2", se2_plus), ("se3", se3_plus)):
        cols = [v for v, k in enumerate(kinds) if k == kind]
        if cols:
            d = 3 if kind == "se2" else 6
            idx = torch.as_tensor(np.asarray(cumsum)[cols][:, None] + np.arange(d)[None, :])
            out[idx] = fn(state[idx], dx[idx])
    for v, k in enumerate(kinds):
        if k == "euclidean":
            out[cumsum[v]:cumsum[v + 1]] = state[cumsum[v]:cumsum[v + 1]] + dx[cumsum[v]:cumsum[v + 1]]
    return out.numpy()


def dense_system(cumsum, v0, v1, J0, J1, sigma_inv, err, unary_vertex=None, unary_factor=None, unary_error=None):
    """Lambda = sum J^T Omega J and eta = sum J^T Omega err, dense, plus U^T U and the unary error at the anchor
    (NonlinearSolver_Lambda_Base.h:1551-1567)."""
    n = int(cumsum[-1])
    lam, eta = np.zeros((n, n)), np.zeros(n)
    for e in range(len(v0)):
        J = np.zeros((J0.shape[1], n))
        J[:, cumsum[v0[e]]:cumsum[v0[e] + 1]] = J0[e]
        J[:, cumsum[v1[e]]:cumsum[v1[e] + 1]] = J1[e]
        lam += J.T @ sigma_inv[e] @ J
        eta += J.T @ sigma_inv[e] @ err[e]
    if unary_vertex is not None:
        s = slice(cumsum[unary_vertex], cumsum[unary_vertex + 1])
        lam[s, s] += unary_factor.T @ unary_factor
        if unary_error is not None:
            eta[s] += unary_error
    return lam, eta
