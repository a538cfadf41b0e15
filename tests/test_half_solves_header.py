"""Solve_L_Columns / Solve_Lt_Columns of the header binding (include/slam/LinearSolver_HIP.h), on CLinearSolver_HIP and on
CLinearSolver_Schur_HIP: the members exist once per class, compile against the reference's headers, and -- linked with the
reference's block matrix that build() compiles into oracle/_ref, with the stand-ins for the C ABI (tests/capi_standins.h)
and a stand-in slampp_hip_solve_half_columns of the driver's own (tests/half_solves_header_driver.cpp) -- hand the caller's
column-major matrix over in one host call with the right n_half, return false with the library's message where it refuses
(no kept factor, Schur mode), and throw on the other failure statuses.  The driver is a stand-alone program.  Skip where the
reference's sources (or the archives built from them) are not present."""
import os
import re
import subprocess

from header_util import ROOT, _compiler_flags, syntax_check

TU = r"""
#include "slam/LinearSolver_HIP.h"
bool halves_of_both(CLinearSolver_HIP &r_sparse, CLinearSolver_Schur_HIP<> &r_schur, Eigen::MatrixXd &r_columns)
{
	return r_sparse.Solve_L_Columns(r_columns) && r_sparse.Solve_Lt_Columns(r_columns) &&
		r_schur.Solve_L_Columns(r_columns) && r_schur.Solve_Lt_Columns(r_columns) &&
		r_sparse.r_s_Half_Solve_Refusal().empty() && r_schur.r_s_Half_Solve_Refusal().empty();
}
"""


def test_header_declares_the_half_solves():
    """(runs everywhere: the members on both classes, one library call behind them, and the C entry points)"""
    text = open(os.path.join(ROOT, "include", "slam", "LinearSolver_HIP.h")).read()
    for member in ("Solve_L_Columns", "Solve_Lt_Columns"):
        assert len(re.findall(r"bool\s+" + member + r"\s*\(\s*Eigen::MatrixXd\s*&\s*r_columns\s*\)", text)) == 2, member
    assert len(re.findall(r"slampp_hip_solve_half_columns\s*\(\s*m_p_solver\s*,", text)) == 1
    capi = open(os.path.join(ROOT, "include", "slampp_hip.h")).read()
    assert "slampp_hip_solve_half_columns(" in capi and "slampp_hip_solve_half_columns_device_async(" in capi
    assert re.search(r"#define\s+SLAMPP_HIP_HALF_FORWARD\s+0\b", capi) and re.search(r"#define\s+SLAMPP_HIP_HALF_BACKWARD\s+1\b", capi)
    assert re.search(r"#define\s+SLAMPP_HIP_GRAM_MAX_COLUMNS\s+48\b", capi) and "slampp_hip_gram_device_async(" in capi


def test_half_solves_compile_on_both_classes(tmp_path):
    syntax_check(tmp_path, "half_solves_tu.cpp", TU)


def test_half_solves_hand_the_matrix_over_in_one_call(tmp_path):
    flags, libs = _compiler_flags(True)
    exe = tmp_path / "half_solves_header_driver"
    cmd = ["g++"] + flags + [os.path.join(ROOT, "tests", "half_solves_header_driver.cpp"), "-o", str(exe)] + libs + ["-lrt", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:] + r.stderr[-4000:]
