#!/usr/bin/env python3
"""Generates tests/golden/lm/{se2,se3,ba}.npz: the reference's CNonlinearSolver_Lambda_LM (CLinearSolver_CholMod, no Schur
complement) on the graphs of tests/golden/linearize/ from their own states, through tests/lm_golden_driver.cpp (built here with
the include paths and archives of oracle/Makefile.ref, as tests/golden/make_linearize_golden.py builds its driver).  Run where
the reference is present:

    python -c "import __graft_entry__ as g; g.build()" && python tests/golden/make_lm_golden.py

Per fixture, for n_max = 1 .. 8: ``chi2`` [8] and ``states`` [8, n_scalars] after Optimize(n_max, f_min_dx_norm), ``n_iterations``
[8] as the solver counted them, and once ``f_min_dx_norm`` (that of tests/lm_model.LOOPS), ``unary_vertex``, ``unary_factor``
[d, d] and ``unary_error`` [d]: the anchor the reference's system made for itself, so that a run compared with these uses the
same.  Data only; no reference source text is stored."""
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

N_MAX_RUNS = 8


def build_driver(td):
    v = header_util._makefile_vars()
    libs = v["REFLIBS"].split()
    assert all(os.path.isfile(a) for a in libs), "build the reference's archives first (build())"
    flags = ["-w"] + v["OPT"].split() + v["CDEFS"].split() + v["CHOLMOD_DEFS"].split() + v["INC"].split()
    exe = os.path.join(td, "lm_golden_driver")
    subprocess.run(["g++"] + flags + [os.path.join(ROOT, "tests", "lm_golden_driver.cpp"), "-o", exe] + libs + ["-lrt", "-lm"], check=True)
    return exe


def main():
    with tempfile.TemporaryDirectory() as td:
        exe = build_driver(td)
        for kind in M.KINDS:
            fx = M.load_fixture(kind)
            f_min_dx_norm = L.LOOPS[kind][1]
            src, dst = os.path.join(td, kind + ".in"), os.path.join(td, kind + ".out")
            M.write_driver_input(src, kind, fx)
            r = subprocess.run([exe, src, dst, repr(f_min_dx_norm)], capture_output=True, text=True)
            assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
            out = np.fromfile(dst)
            n = len(fx["state"])
            vertex, d = int(out[0]), int(out[1])
            factor = out[2:2 + d * d].reshape(d, d).T.copy()
            error = out[2 + d * d:2 + d * d + d].copy()
            runs = out[2 + d * d + d:].reshape(N_MAX_RUNS, 2 + n)
            os.makedirs(os.path.join(HERE, "lm"), exist_ok=True)
            path = os.path.join(HERE, "lm", f"{kind}.npz")
            np.savez_compressed(path, f_min_dx_norm=np.float64(f_min_dx_norm), unary_vertex=np.int64(vertex), unary_factor=factor,
                                unary_error=error, chi2=runs[:, 0].copy(), n_iterations=runs[:, 1].astype(np.int64), states=runs[:, 2:].copy())
            print(f"lm_{kind}: unary factor {d} x {d} on vertex {vertex} (diagonal {np.diag(factor)}), iterations {runs[:, 1].astype(int)}, "
                  f"chi2 {runs[:, 0]} -> {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
