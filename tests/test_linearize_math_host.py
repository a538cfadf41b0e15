"""The arithmetic of the linearize and state_plus kernels (slam_plus_plus_amd/csrc/linearize_math.h) compiled for the host
and run on the three fixtures, against the exact model: the bound of the GPU test, 1e-10 rel-inf of the largest entry of each
array over the edge set, here without a GPU.  It includes the zero rotation and the angles 1e-9, 1e-5 and 1e-3 on either side
of the series threshold, and the two states above pi."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import linearize_model as M
from golden_util import rel_inf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("linearize_math") / "linearize_math_driver"
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-w", "-I" + os.path.join(ROOT, "slam_plus_plus_amd", "csrc"),
                        os.path.join(ROOT, "tests", "linearize_math_driver.cpp"), "-o", str(exe), "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("kind", M.KINDS)
def test_kernel_arithmetic_matches_the_model(driver, tmp_path, kind):
    fx = M.load_fixture(kind)
    d0, d1, rd = M.EDGE_SHAPES[kind]
    n_edges, n = len(fx["v0"]), len(fx["state"])
    M.write_driver_input(tmp_path / "in.bin", kind, fx)
    r = subprocess.run([str(driver), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    out = np.fromfile(tmp_path / "out.bin")
    sizes = [n_edges * rd * d0, n_edges * rd * d1, n_edges * rd, n, n]
    assert out.size == sum(sizes)
    J0, J1, err, plus, minus = np.split(out, np.cumsum(sizes)[:-1])
    J0 = J0.reshape(n_edges, d0, rd).transpose(0, 2, 1)
    J1 = J1.reshape(n_edges, d1, rd).transpose(0, 2, 1)
    _, err_m, J0_m, J1_m = M.fixture_model(kind)
    assert rel_inf(err.reshape(n_edges, rd), err_m) < TOL
    assert rel_inf(J0, J0_m) < TOL and rel_inf(J1, J1_m) < TOL
    kinds = M.vertex_kinds(kind, fx)
    assert rel_inf(plus, M.state_plus(kinds, fx["state"], fx["cumsum"], fx["dx"])) < TOL
    assert rel_inf(minus, M.state_plus(kinds, fx["state"], fx["cumsum"], fx["dx"], -1.0)) < TOL
    assert rel_inf(plus, fx["state_plus"]) < TOL and rel_inf(minus, fx["state_minus"]) < TOL and rel_inf(err.reshape(n_edges, rd), fx["err"]) < TOL
