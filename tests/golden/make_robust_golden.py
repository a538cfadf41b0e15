#!/usr/bin/env python3
"""Generates tests/golden/robust/{kernels,se3_outliers}.npz through tests/robust_golden_driver.cpp (built here with the include
paths and archives of oracle/Makefile.ref, as tests/golden/make_lm_golden.py builds its driver).  Run where the reference is
present:

    python -c "import __graft_entry__ as g; g.build()" && python tests/golden/make_robust_golden.py

kernels.npz: per loss function (``huber``, ``cauchy``, ``tukey``, ``welsch``) an array [2, 1 + 2 * 8]: for the reference's default
parameter and for a = 1 a row (a, s_0, w_0, .. s_7, w_7) of the reference's operator () on the grid s = 0, a / 2, the double below
a, a, the double above a, 2 a, 10 a, 1e3 a; ``vectors`` [6, 6] and ``vector_weights`` [6]: f_RobustWeight of
CRobustify_ErrorNorm_Default<CCTFraction<30, 100>, CHuberLossd>.

se3_outliers.npz: the graph and start state of tests/golden/linearize/se3.npz with the measurements of edges 3, 10, .. 52
perturbed (tests/robust_model.outlier_measurements: the translation by N(0, 0.8), the rotation by N(0, 0.3), default_rng(robust_model.OUTLIER_SEED)):
``z`` [55, 6] the measurements, ``weights`` [55] every CEdgePose3D's own f_RobustWeight at the start state, and what
tests/golden/lm/se3.npz records of the reference's CNonlinearSolver_Lambda_LM for Optimize(n_max, f_min_dx_norm), n_max = 1 .. 8:
``chi2`` [8], ``states`` [8, 240], ``n_iterations`` [8], ``f_min_dx_norm``, ``unary_vertex``, ``unary_factor``, ``unary_error``.
The four conditions the fixture must meet are asserted here (and again by tests/test_robust_model_host.py); were one to fail,
the seed is what changes.  Data only; no reference source text is stored."""
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
import linearize_model as M  # noqa: E402
import lm_model as L  # noqa: E402
import robust_model as R  # noqa: E402

N_MAX_RUNS, N_GRID, N_VECTORS = 8, 8, 6
SEED = R.OUTLIER_SEED


def build_driver(td):
    v = header_util._makefile_vars()
    libs = v["REFLIBS"].split()
    assert all(os.path.isfile(a) for a in libs), "build the reference's archives first (build())"
    flags = ["-w"] + v["OPT"].split() + v["CDEFS"].split() + v["CHOLMOD_DEFS"].split() + v["INC"].split()
    exe = os.path.join(td, "robust_golden_driver")
    subprocess.run(["g++"] + flags + [os.path.join(ROOT, "tests", "robust_golden_driver.cpp"), "-o", exe] + libs + ["-lrt", "-lm"], check=True)
    return exe


def run_driver(args):
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def check_conditions(g, runs):
    """The fixture's four conditions (tests/test_robust_model_host.py asserts them again)."""
    w = g["weights"]
    assert np.sum(w < 0.9) >= 5 and np.sum(w == 1) >= 5, w
    accepted = np.concatenate([r["trace"][:L.compared_rounds(r), L.T_ACCEPTED] for r in runs])
    rho = np.concatenate([r["trace"][:L.compared_rounds(r), L.T_RHO] for r in runs])
    assert np.abs(rho).min() >= 0.02, np.abs(rho).min()
    assert accepted.min() == 0 and accepted.max() == 1
    assert [int(r["scalars"][L.N_ROUNDS]) for r in runs] == list(g["n_iterations"]), ([r["scalars"][L.N_ROUNDS] for r in runs], g["n_iterations"])


def main():
    os.makedirs(R.GOLDEN, exist_ok=True)
    with tempfile.TemporaryDirectory() as td:
        exe = build_driver(td)
        dst = os.path.join(td, "kernels.out")
        run_driver([exe, "kernels", dst])
        out = np.fromfile(dst)
        row = 1 + 2 * N_GRID
        tables = out[:8 * row].reshape(4, 2, row)
        vectors = out[8 * row:].reshape(N_VECTORS, 7)
        path = os.path.join(R.GOLDEN, "kernels.npz")
        np.savez_compressed(path, huber=tables[0], cauchy=tables[1], tukey=tables[2], welsch=tables[3], vectors=vectors[:, :6].copy(),
                            vector_weights=vectors[:, 6].copy())
        print(f"kernels: parameters {tables[:, :, 0].tolist()}, vector weights {vectors[:, 6]} -> {os.path.getsize(path) / 1024:.1f} KiB")

        fx = dict(M.load_fixture("se3"))
        fx["z"] = R.outlier_measurements(SEED)
        f_min_dx_norm = L.LOOPS["se3"][1]
        src, dst = os.path.join(td, "se3.in"), os.path.join(td, "se3.out")
        M.write_driver_input(src, "se3", fx)
        run_driver([exe, "lm", src, dst, repr(f_min_dx_norm)])
        out = np.fromfile(dst)
        n, n_edges = len(fx["state"]), len(fx["v0"])
        weights, out = out[:n_edges].copy(), out[n_edges:]
        vertex, d = int(out[0]), int(out[1])
        factor = out[2:2 + d * d].reshape(d, d).T.copy()
        error = out[2 + d * d:2 + d * d + d].copy()
        runs = out[2 + d * d + d:].reshape(N_MAX_RUNS, 2 + n)
        path = os.path.join(R.GOLDEN, "se3_outliers.npz")
        np.savez_compressed(path, z=fx["z"], weights=weights, f_min_dx_norm=np.float64(f_min_dx_norm), unary_vertex=np.int64(vertex),
                            unary_factor=factor, unary_error=error, chi2=runs[:, 0].copy(), n_iterations=runs[:, 1].astype(np.int64),
                            states=runs[:, 2:].copy())
        print(f"se3_outliers: {np.sum(weights < 0.9)} weights below 0.9 (the least {weights.min():.3f}), {np.sum(weights == 1)} equal to 1; "
              f"iterations {runs[:, 1].astype(int)}, chi2 {runs[:, 0]} -> {os.path.getsize(path) / 1024:.1f} KiB")
    R._cache.clear()
    check_conditions(R.load_golden("se3_outliers"), R.outlier_runs())
    print("the fixture's four conditions hold")


if __name__ == "__main__":
    main()
