"""The yardsticks of the differentiable solve (slam_plus_plus_amd/torch_solve.py) on the CPU: dense_from_packed against
scipy, pattern_outer_reference against the adjoint identity <v, P(a, b)> = a^T M(v) b and against the values gradient of
dense torch.linalg.solve autograd; and the host lookup tables of the outer-product kernel under sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from slam_plus_plus_amd.torch_solve import dense_from_packed, pattern_outer_reference
from golden_util import golden_names, dump_names, load_golden, load_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam_plus_plus_amd", "csrc")
SYSTEMS = golden_names() + dump_names()


def _load(name):
    return load_dump(name)[0] if name.startswith("dump_") else load_golden(name)[0]


@pytest.mark.parametrize("name", SYSTEMS)
def test_dense_from_packed_is_the_matrix_scipy_builds(name):
    lam = _load(name)
    M = dense_from_packed(lam, torch.from_numpy(lam.values)).numpy()
    assert np.array_equal(M, lam.to_scipy().toarray())
    assert np.array_equal(M, M.T)


@pytest.mark.parametrize("name", SYSTEMS)
def test_reference_outer_product_is_the_adjoint_of_the_product(name):
    lam = _load(name)
    rng = np.random.default_rng(3)
    a, b, v = rng.standard_normal(lam.n_scalars), rng.standard_normal(lam.n_scalars), rng.standard_normal(lam.values.shape[0])
    M = dense_from_packed(lam, torch.from_numpy(v)).numpy()      # (v is any vector: M(v) is linear in it)
    P = pattern_outer_reference(lam, a, b)
    lhs, rhs = float(v @ P), float(a @ M @ b)
    terms = float(np.abs(v) @ pattern_outer_reference(lam, np.abs(a), np.abs(b)))
    print(f"{name}: <v, P(a, b)> = {lhs:.15e}, a^T M(v) b = {rhs:.15e}, sum |terms| = {terms:.3e}")
    # two orders of the same sum of n_values products (each product rounded at most three times)
    assert abs(lhs - rhs) <= 4 * v.shape[0] * np.finfo(float).eps * terms
    assert np.array_equal(pattern_outer_reference(lam, a, b, -2.0), -2.0 * P)


@pytest.mark.parametrize("name", ["chain6_n60", "manhattan_n150", "sphere_8x8", "ba_12x150_venice"])
def test_reference_gradient_is_the_one_of_dense_autograd(name):
    lam = _load(name)
    w = torch.from_numpy(np.random.default_rng(4).standard_normal(lam.n_scalars))
    values = torch.from_numpy(lam.values).clone().requires_grad_(True)
    eta = torch.from_numpy(lam.rhs).clone().requires_grad_(True)
    x = torch.linalg.solve(dense_from_packed(lam, values), eta)
    (w @ x).backward()
    g = np.linalg.solve(dense_from_packed(lam, values.detach()).numpy(), w.numpy())
    v_bar = pattern_outer_reference(lam, g, x.detach().numpy(), -1.0)
    err_v = float(np.abs(v_bar - values.grad.numpy()).max() / np.abs(values.grad.numpy()).max())
    err_eta = float(np.abs(g - eta.grad.numpy()).max() / np.abs(g).max())
    print(f"{name}: values gradient rel-inf {err_v:.2e}, eta gradient rel-inf {err_eta:.2e}")
    assert err_v < 1e-12 and err_eta < 1e-12


def test_lookup_tables_are_right_and_clean_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "pattern_outer_tables_driver"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I" + CSRC,
           os.path.join(ROOT, "tests", "pattern_outer_tables_driver.cpp"), os.path.join(CSRC, "pattern_outer_tables.cpp"),
           "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "sanitizer" in (build.stderr or "").lower() and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == 7 and all(l.endswith(" ok") for l in lines), run.stdout
