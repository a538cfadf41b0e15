"""The arithmetic of the pose-landmark and stereo edges of the linearize kernel (slam_plus_plus_amd/csrc/linearize_math.h)
compiled for the host with plain g++ and run on the three fixtures of tests/golden/landmark/, against the exact model of
tests/landmark_model.py: the bound of the GPU test, 1e-10 rel-inf of the largest entry of each array over the edge set, here
without a GPU.  The three close edges of lm2d (range 0, 5e-6 and 2e-5: on either side of the range clamp) have the bits of
the reference's closed form evaluated in the order of the C code.

Then the same driver as a stand-alone program under -fsanitize=address,undefined on the same inputs: nothing is loaded into
Python and nothing is preloaded."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import landmark_model as L
from golden_util import rel_inf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10


def build_driver(directory, sanitize):
    """Compiles the driver (None where there is no g++ or, with ``sanitize``, no sanitizer runtime)."""
    if shutil.which("g++") is None:
        return None
    exe = os.path.join(str(directory), "landmark_math_driver")
    cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "slam_plus_plus_amd", "csrc"),
           os.path.join(ROOT, "tests", "landmark_math_driver.cpp"), "-o", exe, "-lm"]
    if sanitize:
        cmd[1:2] = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if sanitize and build.returncode != 0 and "sanitizer" in (build.stderr or "").lower() and "cannot find" in build.stderr:
        return None
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = build_driver(tmp_path_factory.mktemp("landmark_math"), False)
    if exe is None:
        pytest.skip("no g++")
    return exe


@pytest.fixture(scope="module")
def sanitized_driver(tmp_path_factory):
    exe = build_driver(tmp_path_factory.mktemp("landmark_math_sanitized"), True)
    if exe is None:
        pytest.skip("no g++ or no sanitizer runtime")
    return exe


def run_driver(exe, directory, name, env=None):
    fx = L.load_fixture(name)
    d0, d1, rd = L.EDGE_SHAPES[name]
    n_edges = len(fx["v0"])
    src, dst = os.path.join(str(directory), name + ".in"), os.path.join(str(directory), name + ".out")
    L.write_driver_input(src, name, fx)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    out = np.fromfile(dst)
    sizes = [n_edges * rd * d0, n_edges * rd * d1, n_edges * rd]
    assert out.size == sum(sizes)
    J0, J1, err = np.split(out, np.cumsum(sizes)[:-1])
    return (J0.reshape(n_edges, d0, rd).transpose(0, 2, 1), J1.reshape(n_edges, d1, rd).transpose(0, 2, 1), err.reshape(n_edges, rd)), r


def check_against_the_model(name, J0, J1, err):
    fx = L.load_fixture(name)
    _, err_m, J0_m, J1_m = L.fixture_model(name)
    assert rel_inf(err, err_m) < TOL and rel_inf(err, fx["err"]) < TOL
    assert rel_inf(J0, J0_m) < TOL and rel_inf(J1, J1_m) < TOL
    if name == "lm2d":       # the close edges: the model's 2D Jacobians are the closed form in C order
        assert rel_inf(J0[:-3], J0_m[:-3]) < TOL and rel_inf(J1[:-3], J1_m[:-3]) < TOL      # (without the 1e5 of the clamped ones)
        assert np.array_equal(J0[-3:], J0_m[-3:]) and np.array_equal(J1[-3:], J1_m[-3:])
        assert np.array_equal(err[-3:, 0], err_m[-3:, 0])
        assert np.abs(J0[-3]).max() == 1.0 and np.abs(J1[-3]).max() == 0.0 and np.abs(J1[-2]).max() > 1e4


@pytest.mark.parametrize("name", L.NAMES)
def test_kernel_arithmetic_matches_the_model(driver, tmp_path, name):
    (J0, J1, err), _ = run_driver(driver, tmp_path, name)
    check_against_the_model(name, J0, J1, err)


@pytest.mark.parametrize("name", L.NAMES)
def test_kernel_arithmetic_is_clean_under_sanitizers(sanitized_driver, tmp_path, name):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SLAMPP_HIP")}
    (J0, J1, err), r = run_driver(sanitized_driver, tmp_path, name, dict(env, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    check_against_the_model(name, J0, J1, err)
