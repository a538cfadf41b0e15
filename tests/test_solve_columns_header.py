"""Solve_Again_Columns of the header binding (include/slam/LinearSolver_HIP.h), on CLinearSolver_HIP and on
CLinearSolver_Schur_HIP: the member compiles against the reference's headers, and -- linked with the reference's block
matrix that build() compiles into oracle/_ref, with the stand-ins for the C ABI (tests/capi_standins.h) and a stand-in
slampp_hip_solve_columns that checks the pointer, the leading dimension, the number of columns and the row of every entry
it is handed (tests/solve_columns_header_driver.cpp) -- hands the caller's column-major matrix over in one host call where
the library's order is lambda's own, permutes the rows by blocks where it is not (the guided ordering of the Schur class),
goes to the class's sparse solver where lambda has no landmark part, and throws on every failure status.  The driver is a
stand-alone program.  Skip where the reference's sources (or the archives built from them) are not present."""
import os
import re
import subprocess

from header_util import ROOT, _compiler_flags, syntax_check

TU = r"""
#include "slam/LinearSolver_HIP.h"
bool columns_of_both(CLinearSolver_HIP &r_sparse, CLinearSolver_Schur_HIP<> &r_schur, Eigen::MatrixXd &r_eta_columns)
{
	return r_sparse.Solve_Again_Columns(r_eta_columns) && r_schur.Solve_Again_Columns(r_eta_columns);
}
"""


def test_header_declares_solve_again_columns():
    """(runs everywhere: the member on both classes under a name of its own, and the C entry points)"""
    text = open(os.path.join(ROOT, "include", "slam", "LinearSolver_HIP.h")).read()
    assert len(re.findall(r"bool\s+Solve_Again_Columns\s*\(\s*Eigen::MatrixXd\s*&\s*r_eta_columns\s*\)", text)) == 2
    assert re.search(r"slampp_hip_solve_columns\s*\(\s*m_p_solver\s*,", text)
    capi = open(os.path.join(ROOT, "include", "slampp_hip.h")).read()
    assert "slampp_hip_solve_columns(" in capi and "slampp_hip_solve_columns_device_async(" in capi
    assert re.search(r"#define\s+SLAMPP_HIP_SOLVE_MAX_COLUMNS\s+256\b", capi)
    assert "slampp_hip_pattern_outer_sum_device_async(" in capi


def test_solve_again_columns_compiles_on_both_classes(tmp_path):
    syntax_check(tmp_path, "solve_columns_tu.cpp", TU)


def test_solve_again_columns_hands_over_the_library_order_in_one_call(tmp_path):
    flags, libs = _compiler_flags(True)
    exe = tmp_path / "solve_columns_header_driver"
    cmd = ["g++"] + flags + [os.path.join(ROOT, "tests", "solve_columns_header_driver.cpp"), "-o", str(exe)] + libs + ["-lrt", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:] + r.stderr[-4000:]
