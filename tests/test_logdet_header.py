"""Log_Determinant of the header binding (include/slam/LinearSolver_HIP.h), on CLinearSolver_HIP, on
CLinearSolver_Schur_HIP and through the CLinearSolver_Schur<CLinearSolver_HIP, ..> specialization: the members compile
against the reference's headers, and -- linked with the reference's block matrix that build() compiles into oracle/_ref,
with the stand-ins for the C ABI (tests/capi_standins.h) and a stand-in slampp_hip_logdet that checks the place of every
value it is handed (tests/logdet_header_driver.cpp) -- hand the gathered values over in the library's order (the guided
ordering for the Schur class), pass the result through, answer false where the matrix is not positive definite and throw
on every other status.  Skip where the reference's sources (or the archives built from them) are not present."""
import os
import re
import subprocess

from header_util import ROOT, _compiler_flags, syntax_check

TU = r"""
#include "slam/LinearSolver_HIP.h"
struct TSystemTypes { typedef void _TyVertexTypelist; typedef void _TyEdgeTypelist; typedef void _TyHessianMatrixBlockList; };
bool logdet_of_all(CLinearSolver_HIP &r_sparse, CLinearSolver_Schur_HIP<> &r_schur, const CUberBlockMatrix &r_lambda)
{
	CLinearSolver_Schur<CLinearSolver_HIP, void, TSystemTypes> nonlinear_solvers_schur(r_sparse); // what the reference's nonlinear solvers hold
	double f_a, f_b, f_c;
	return r_sparse.Log_Determinant(f_a, r_lambda) && r_schur.Log_Determinant(f_b, r_lambda) &&
		nonlinear_solvers_schur.Log_Determinant(f_c, r_lambda);
}
"""


def test_header_declares_log_determinant():
    """(runs everywhere: the member on both classes, and the C entry points it calls)"""
    text = open(os.path.join(ROOT, "include", "slam", "LinearSolver_HIP.h")).read()
    assert len(re.findall(r"bool\s+Log_Determinant\s*\(\s*double\s*&\s*r_f_logdet\s*,\s*const\s+CUberBlockMatrix\s*&", text)) == 2
    assert re.search(r"slampp_hip_logdet\s*\(\s*m_p_solver\s*,\s*m_p_values\s*,\s*0\s*,", text)      # b_reuse_factor = 0
    capi = open(os.path.join(ROOT, "include", "slampp_hip.h")).read()
    assert "slampp_hip_logdet(" in capi and "slampp_hip_logdet_device_async(" in capi


def test_log_determinant_compiles_on_both_classes_and_the_specialization(tmp_path):
    syntax_check(tmp_path, "logdet_tu.cpp", TU)


def test_log_determinant_hands_over_the_library_order_and_passes_the_result(tmp_path):
    flags, libs = _compiler_flags(True)
    exe = tmp_path / "logdet_header_driver"
    cmd = ["g++"] + flags + [os.path.join(ROOT, "tests", "logdet_header_driver.cpp"), "-o", str(exe)] + libs + ["-lrt", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:] + r.stderr[-4000:]
