#!/usr/bin/env python3
"""Generates tests/golden/linearize/{se2,se3,ba}.npz: small graphs with explicit vertex states, evaluated by the reference's
own vertex and edge classes through tests/linearize_golden_driver.cpp (built here with the include paths and archives of
oracle/Makefile.ref, as tests/header_util.py builds the header drivers).  They lie in a directory of their own because
tests/golden_util.py takes every .npz directly under tests/golden/ without one of its prefixes for a linear system with
reference solutions.  Run where the reference is present:

    python -c "import __graft_entry__ as g; g.build()" && python tests/golden/make_linearize_golden.py

Per fixture: the inputs (``state``, ``cumsum``, ``v0``, ``v1``, ``z``, ``sigma_inv``, ``params`` for BA, ``dx``) and, from the
reference: ``J0``, ``J1`` (per edge rd x d, stored row-major [E, rd, d]), ``expectation``, ``err``, ``chi2`` (the sum of the
edges' f_Chi_Squared_Error) and the states after Operator_Plus(dx) / Operator_Minus(dx) of every vertex (``state_plus``,
``state_minus``).  Data only; no reference source text is stored.

SE(2), SE(3): 40 poses and the 55 edges of `ref_harness lambda_dump` (odometry, doubled and longer-range edges, four edges from
the later vertex back to an earlier one).  The SE(3) rotations follow one slowly turning axis with prescribed angles: zero,
1e-9, 1e-5, 1e-3, several between 1 and 3 and two above pi (3.5 and 5, which the reference folds through w < 0); the SE(2)
headings are kept modulo 2 pi with the sign of the turn, so that differences of neighbours wrap.  BA: 6 cameras on a ring, 40
points, each seen by 2 to 4 cameras, every camera with its own intrinsics and radial coefficient.

The composite rotation Log(R0^T R1) and the error rotation of every SE(3) edge must stay below pi - 0.2 (the logarithm is
ill-conditioned at pi, for the reference as well): asserted below, naming the edge."""
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import header_util  # noqa: E402
import linearize_model as M  # noqa: E402  (used for the logarithm and the measurements only; the outputs are the reference's)
import torch  # noqa: E402

KINDS = {"se2": 1, "se3": 2, "ba": 3}


def build_driver(td):
    v = header_util._makefile_vars()
    libs = v["REFLIBS"].split()
    assert all(os.path.isfile(a) for a in libs), "build the reference's archives first (build())"
    flags = ["-w"] + v["OPT"].split() + v["CDEFS"].split() + v["CHOLMOD_DEFS"].split() + v["INC"].split()
    exe = os.path.join(td, "linearize_golden_driver")
    subprocess.run(["g++"] + flags + [os.path.join(ROOT, "tests", "linearize_golden_driver.cpp"), "-o", exe] + libs + ["-lrt", "-lm"],
                   check=True)
    return exe


def pose_edges(n):
    """The edge pattern of Lambda_Dump (oracle/ref_harness.cpp)."""
    v0, v1 = [], []
    for i in range(1, n):
        v0.append(i - 1), v1.append(i)
        if i >= 6 and i % 5 == 0:
            v0.extend([i - 1, i - 3]), v1.extend([i, i])
        if i >= 8 and i % 7 == 0:
            v0.append(i), v1.append(i - 4)
    return np.array(v0, np.int64), np.array(v1, np.int64)


def informations(rng, n_edges, rd):
    """Symmetric positive definite, not diagonal, different for every edge."""
    out = np.empty((n_edges, rd, rd))
    for e in range(n_edges):
        N = rng.normal(0, 1, (rd, rd))
        out[e] = np.diag(40.0 + 3 * np.arange(rd) + rng.uniform(0, 5, rd)) + 0.5 * (N + N.T)
    return out


def se2_case(rng):
    n = 40
    v0, v1 = pose_edges(n)
    heading = np.fmod(0.9 * np.arange(n), 2 * math.pi)          # drops by 2 pi between neighbours
    heading[20:] = -np.fmod(0.7 * np.arange(20, n), 2 * math.pi)  # and turns the other way
    state = np.stack([np.arange(n) + rng.normal(0, 0.1, n), 0.5 * np.sin(np.arange(n)) + rng.normal(0, 0.1, n), heading], 1)
    x0, x1 = torch.from_numpy(state[v0]), torch.from_numpy(state[v1])
    h = M.se2_expectation(x0, x1).numpy()
    z = h + rng.normal(0, 0.05, h.shape)
    z[:, 2] = np.arctan2(np.sin(z[:, 2]), np.cos(z[:, 2]))       # measured angles in (-pi, pi]: z - h is off by a turn where h wrapped
    return dict(state=state.ravel(), cumsum=3 * np.arange(n + 1), v0=v0, v1=v1, z=z, sigma_inv=informations(rng, len(v0), 3),
                params=np.zeros(0), n_cams=0)


SE3_ANGLES = [0.0, 1e-9, 1e-5, 1e-3, 0.4, 0.8, 1.2, 1.7, 2.2, 2.7, 3.5, 4.2 - 2 * math.pi, 5.0, 5.6 - 2 * math.pi]


def se3_case(rng):
    n = 40
    v0, v1 = pose_edges(n)
    angles = list(SE3_ANGLES)
    total = 5.6
    while len(angles) < n:
        total += 0.45
        angles.append(math.remainder(total, 2 * math.pi))       # principal from here on
    i = np.arange(n)
    axis = np.stack([1 + 0.15 * np.sin(0.3 * i), 0.4 + 0.15 * np.cos(0.2 * i), -0.3 + 0.1 * np.sin(0.5 * i)], 1)
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    rot = axis * np.array(angles)[:, None]
    t = np.stack([i + rng.normal(0, 0.1, n), 0.5 * np.sin(i) + rng.normal(0, 0.1, n), 0.1 * i + rng.normal(0, 0.1, n)], 1)
    state = np.concatenate([t, rot], 1)
    x0, x1 = torch.from_numpy(state[v0]), torch.from_numpy(state[v1])
    h = M.se3_expectation(x0, x1)
    noise = torch.from_numpy(rng.normal(0, 0.05, h.shape))
    z = torch.cat([h[:, :3] + noise[:, :3], M.so3_log(M.so3_exp(h[:, 3:]) @ M.so3_exp(noise[:, 3:]))], 1).numpy()
    return dict(state=state.ravel(), cumsum=6 * np.arange(n + 1), v0=v0, v1=v1, z=z, sigma_inv=informations(rng, len(v0), 6),
                params=np.zeros(0), n_cams=0)


def ba_case(rng):
    n_cams, n_pts = 6, 40
    cams = np.empty((n_cams, 6))
    for c in range(n_cams):
        a = 2 * math.pi * c / n_cams
        C = np.array([8 * math.cos(a), 8 * math.sin(a), 1.5 * math.sin(3 * a) + 0.3])
        zc = -C / np.linalg.norm(C)
        xc = np.cross([0, 0, 1.0], zc)
        xc /= np.linalg.norm(xc)
        R = np.stack([xc, np.cross(zc, xc), zc])                 # world -> camera
        cams[c, :3] = -R @ C
        cams[c, 3:] = M.so3_log(torch.from_numpy(R)).numpy()
    pts = rng.normal(0, 1, (n_pts, 3)) * [1.5, 1.5, 1.0]
    params = np.stack([500 + rng.uniform(-20, 20, n_cams), 500 + rng.uniform(-20, 20, n_cams), 320 + rng.uniform(-5, 5, n_cams),
                       240 + rng.uniform(-5, 5, n_cams), rng.uniform(-3e-4, 3e-4, n_cams)], 1)
    v0, v1 = [], []
    for p in range(n_pts):
        for c in sorted(rng.choice(n_cams, size=2 + p % 3, replace=False)):
            v0.append(c), v1.append(n_cams + p)
    v0, v1 = np.array(v0, np.int64), np.array(v1, np.int64)
    K = torch.from_numpy(params[v0])
    z = M.p2c_expectation(torch.from_numpy(cams[v0]), torch.from_numpy(pts[v1 - n_cams]), K).numpy() + rng.normal(0, 0.5, (len(v0), 2))
    cams_est = cams + np.concatenate([rng.normal(0, 0.02, (n_cams, 3)), rng.normal(0, 0.005, (n_cams, 3))], 1)
    pts_est = pts + rng.normal(0, 0.03, pts.shape)
    cumsum = np.concatenate([6 * np.arange(n_cams), 6 * n_cams + 3 * np.arange(n_pts + 1)])
    return dict(state=np.concatenate([cams_est.ravel(), pts_est.ravel()]), cumsum=cumsum, v0=v0, v1=v1, z=z,
                sigma_inv=informations(rng, len(v0), 2) / 40, params=params.ravel(), n_cams=n_cams)


def run_reference(exe, td, kind, case, dx):
    d0, d1, rd = M.EDGE_SHAPES[kind]
    n_edges, n_verts = len(case["v0"]), len(case["cumsum"]) - 1
    src, dst = os.path.join(td, kind + ".in"), os.path.join(td, kind + ".out")
    with open(src, "wb") as f:
        np.array([KINDS[kind], n_verts, n_edges, case["n_cams"]], np.int64).tofile(f)
        for a in (case["state"], case["v0"], case["v1"], case["z"], np.transpose(case["sigma_inv"], (0, 2, 1)), case["params"], dx):
            np.ascontiguousarray(a).tofile(f)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    out = np.fromfile(dst)
    n = len(case["state"])
    sizes = [n_edges * rd * d0, n_edges * rd * d1, n_edges * rd, n_edges * rd, 1, n, n]
    assert out.size == sum(sizes)
    J0, J1, h, err, chi2, plus, minus = np.split(out, np.cumsum(sizes)[:-1])
    return dict(J0=J0.reshape(n_edges, d0, rd).transpose(0, 2, 1).copy(), J1=J1.reshape(n_edges, d1, rd).transpose(0, 2, 1).copy(),
                expectation=h.reshape(n_edges, rd), err=err.reshape(n_edges, rd), chi2=np.float64(chi2[0]), state_plus=plus,
                state_minus=minus)


def main():
    with tempfile.TemporaryDirectory() as td:
        exe = build_driver(td)
        for kind, make, seed in (("se2", se2_case, 31), ("se3", se3_case, 32), ("ba", ba_case, 33)):
            rng = np.random.default_rng(seed)
            case = make(rng)
            dx = rng.normal(0, 0.1, case["state"].shape) if kind != "ba" else rng.normal(0, 0.02, case["state"].shape)
            ref = run_reference(exe, td, kind, case, dx)
            if kind == "se3":
                limit = math.pi - 0.2
                for e in range(len(case["v0"])):
                    a, b = np.linalg.norm(ref["expectation"][e, 3:]), np.linalg.norm(ref["err"][e, 3:])
                    assert a < limit and b < limit, f"SE(3) edge {e} ({case['v0'][e]} -> {case['v1'][e]}): composite rotation {a:.3f}, " \
                                                    f"error rotation {b:.3f}, limit {limit:.3f}"
                norms = np.linalg.norm(case["state"].reshape(-1, 6)[:, 3:], axis=1)
                assert norms[0] == 0 and abs(norms[1] - 1e-9) < 1e-20 and abs(norms[10] - 3.5) < 1e-12 and abs(norms[12] - 5) < 1e-12
            if kind == "se2":
                wrapped = np.abs(case["z"][:, 2] - ref["expectation"][:, 2]) > math.pi
                assert wrapped.sum() >= 3, "no SE(2) angle difference wraps"
            rec = {k: v for k, v in case.items() if k != "n_cams"}
            rec.update(ref, dx=dx, n_cams=np.int64(case["n_cams"]))
            os.makedirs(os.path.join(HERE, "linearize"), exist_ok=True)
            path = os.path.join(HERE, "linearize", f"{kind}.npz")
            np.savez_compressed(path, **rec)
            print(f"linearize_{kind}: verts={len(case['cumsum']) - 1} edges={len(case['v0'])} flipped={int((case['v0'] > case['v1']).sum())} "
                  f"chi2={float(ref['chi2']):.6g} -> {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
