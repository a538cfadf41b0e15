"""The host passes of the cold path on one worker thread and on many must leave the same tables (csrc/host_threads.h).

Every pass gives a worker thread thousands of records (2 048 - 65 536), so at the sizes of this suite all of them run on the
calling thread; only tests/test_fullsize_reference_gpu.py reaches the many-worker paths.  The development knob
SLAMPP_HIP_DEV_HOST_THREAD_GRAIN (with SLAMPP_HIP_DEV=1) replaces every pass' records per thread: at 256 a system of 4 000
landmarks or 2 000 poses gets up to eight workers in every pass.  The passes promise that every record lands where the serial
pass put it, so the same system is solved twice -- plainly and under the knob -- and the results must agree bit for bit.
The knobs are read once per process: every solve is a fresh child process with one handle (no torch in it)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import dataclasses, json, sys
import numpy as np
from slam_plus_plus_amd import synth
from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP, CLinearSolver_Schur_HIP

kind, arg, out = sys.argv[1], sys.argv[2], sys.argv[3]
if kind.startswith("schur"):
    lam = synth.ba(24, 4000, mode=arg.split(":")[0], k=4, seed=11)
    solver = CLinearSolver_Schur_HIP(schur_tiles=int(arg.split(":")[1]))
else:
    lam = synth.pose_chain(n=2000, d=6, seed=11)
    solver = CLinearSolver_HIP()
n, nc = lam.n_bcols, lam.n_matrix_cut
if kind.endswith("below_diagonal"):       # a block below the diagonal, in the last tenth of the columns
    c = n - n // 20
    brow = lam.brow_idx.copy()
    brow[lam.bcol_ptr[c]] = n - 1
    lam = dataclasses.replace(lam, brow_idx=brow)
elif kind.endswith("no_diagonal"):        # a landmark of the last tenth whose last block is not its diagonal block
    c = n - n // 20
    brow = lam.brow_idx.copy()
    brow[lam.bcol_ptr[c + 1] - 1] = c - 1
    lam = dataclasses.replace(lam, brow_idx=brow)
result = {}
try:
    solver.set_option("profile", 1)
    eta = lam.rhs.copy()
    result["ok"] = bool(solver.Solve_PosDef(lam, eta))
    result["phases"] = sorted(solver.profile())
    arrays = {"x": eta}
    if kind == "schur":
        arrays["cams"], arrays["pts"] = solver.Schur_Marginals(lam)
    np.savez(out + ".npz", **arrays)
except Exception as e:
    result["error"] = [type(e).__name__, str(e)]
with open(out + ".json", "w") as f:
    json.dump(result, f)
"""


def run_child(tmp_path, kind, arg, grain):
    """One solve in a process of its own; grain None: as every host application runs it."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SLAMPP_HIP_DEV_") and k != "SLAMPP_HIP_DEV"}
    if grain is not None:
        env.update(SLAMPP_HIP_DEV="1", SLAMPP_HIP_DEV_HOST_THREAD_GRAIN=str(grain))
    out = str(tmp_path / ("plain" if grain is None else "grain%d" % grain))
    r = subprocess.run([sys.executable, "-c", CHILD, kind, arg, out], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    with open(out + ".json") as f:
        result = json.load(f)
    arrays = dict(np.load(out + ".npz")) if os.path.exists(out + ".npz") else {}
    return result, arrays


def assert_same_bits(plain, knob):
    assert sorted(plain) == sorted(knob) and plain
    for name in plain:
        a, b = torch.from_numpy(plain[name]), torch.from_numpy(knob[name])
        assert a.shape == b.shape and torch.equal(a, b), \
            "%s differs: %d of %d entries, largest difference %g" % (name, int((a != b).sum()), a.numel(), float((a - b).abs().max()))


# schur_tiles (as in tests/test_schur_gpu.py): 0 = contribution lists (the counting sort of schur_setup.hip), 1 = runs and
# tiles, 2 = tiles only (the long tracks of "venice" stay with the lists: the hybrid lists of schur_tiles.hip), 3 = runs only.
# "venice": a few hundred different camera lists (the class passes); "uniform": nearly every landmark a class of its own
@pytest.mark.parametrize("visibility,tiles", [("venice", 0), ("venice", 1), ("venice", 2), ("venice", 3), ("uniform", 1)])
def test_schur_analysis_on_many_workers_leaves_the_same_bits(visibility, tiles, tmp_path):
    arg = "%s:%d" % (visibility, tiles)
    r_plain, plain = run_child(tmp_path, "schur", arg, None)
    r_knob, knob = run_child(tmp_path, "schur", arg, 256)
    assert r_plain == r_knob and r_plain.get("ok") is True and "error" not in r_plain, (r_plain, r_knob)
    if visibility == "venice":
        assert ("schur_tiles" in r_plain["phases"]) == bool(tiles), r_plain["phases"]
    assert_same_bits(plain, knob)                      # the solution and the block-diagonal covariances


def test_sparse_analysis_on_many_workers_leaves_the_same_bits(tmp_path):
    r_plain, plain = run_child(tmp_path, "sparse", "-", None)
    r_knob, knob = run_child(tmp_path, "sparse", "-", 256)
    assert r_plain == r_knob and r_plain.get("ok") is True and "error" not in r_plain, (r_plain, r_knob)
    assert_same_bits(plain, knob)


@pytest.mark.parametrize("kind,arg,message", [
    ("sparse_below_diagonal", "-", "set_structure: block outside the upper triangle"),
    ("schur_below_diagonal", "venice:1", "set_structure: block outside the upper triangle"),
    ("schur_no_diagonal", "venice:1", "Schur path: a landmark has no diagonal block")])
def test_malformed_structure_is_refused_alike_on_many_workers(kind, arg, message, tmp_path):
    """The checks of set_structure and of the Schur analysis report through a slot per worker; which slot is looked at first
    decides the message."""
    r_plain, _ = run_child(tmp_path, kind, arg, None)
    r_knob, _ = run_child(tmp_path, kind, arg, 256)
    assert r_plain.get("error") == ["ValueError", message], r_plain
    assert r_knob == r_plain
