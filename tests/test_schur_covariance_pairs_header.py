"""Marginal_Blocks and Joint_Marginal of the Schur class of the header binding (include/slam/LinearSolver_HIP.h:
CLinearSolver_Schur_HIP) compile against the reference's headers, with the include paths and defines oracle/Makefile.ref
builds the drop-in driver with, and -- linked with the reference's block matrix that build() compiles into oracle/_ref
and with stand-ins for the C ABI (tests/schur_covariance_pairs_header_driver.cpp) -- return block (r, c) of lambda's own
order for every pair.  Skip where the reference's sources (or the archives built from them) are not present."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = r"""
#include "slam/LinearSolver_HIP.h"
bool covariance_pairs(CLinearSolver_Schur_HIP<> &r_solver, const CUberBlockMatrix &r_lambda)
{
	std::vector<std::pair<size_t, size_t> > pairs(1, std::make_pair(r_lambda.n_BlockColumn_Num() - 1, size_t(0)));
	std::vector<size_t> block_columns(1, r_lambda.n_BlockColumn_Num() - 1);
	std::vector<Eigen::MatrixXd> blocks;
	Eigen::MatrixXd joint;
	return r_solver.Marginal_Blocks(blocks, r_lambda, pairs) && r_solver.Joint_Marginal(joint, r_lambda, block_columns);
}
"""


def _makefile_vars():
    text = open(os.path.join(ROOT, "oracle", "Makefile.ref")).read()
    out = {}
    for name in ("REF", "OUT", "OPT", "CDEFS", "INC", "CHOLMOD_DEFS"):
        m = re.search(r"^%s\s*[?:]?=\s*(.*)$" % name, text, re.M)
        assert m, name
        out[name] = m.group(1).strip()
    m = re.search(r"^REFLIBS\s*:=\s*((?:.*\\\n)*.*)$", text, re.M)
    assert m, "REFLIBS"
    out["REFLIBS"] = m.group(1).replace("\\\n", " ")
    for name in ("OPT", "CDEFS", "INC", "CHOLMOD_DEFS", "REFLIBS"):
        out[name] = out[name].replace("$(REF)", out["REF"]).replace("$(OUT)", os.path.join(ROOT, out["OUT"]))
    return out


def test_schur_covariance_pair_members_compile(tmp_path):
    v = _makefile_vars()
    if not os.path.isdir(os.path.join(v["REF"], "include", "slam")):
        pytest.skip("the reference's headers are not present")
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = tmp_path / "schur_covariance_pairs_tu.cpp"
    src.write_text(TU)
    cmd = ["g++", "-fsyntax-only", "-w"] + v["OPT"].split() + v["CDEFS"].split() + v["CHOLMOD_DEFS"].split() + \
        ["-I" + os.path.join(ROOT, "include")] + v["INC"].split() + [str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_schur_covariance_pairs_are_the_blocks_of_lambdas_order(tmp_path):
    """Marginal_Blocks at every ordered pair and Joint_Marginal of a mixed set, run on the CPU against stand-ins for the C ABI
    that answer with a known symmetric matrix, for a BA lambda with the cameras first, one the class reorders (pairs reach the
    library turned around) and one without a landmark part (its sparse solver answers)."""
    v = _makefile_vars()
    if not os.path.isdir(os.path.join(v["REF"], "include", "slam")):
        pytest.skip("the reference's headers are not present")
    libs = v["REFLIBS"].split()
    if not all(os.path.isfile(a) for a in libs):
        pytest.skip("the reference's archives have not been built")
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "schur_covariance_pairs_header_driver"
    cmd = ["g++", "-w"] + v["OPT"].split() + v["CDEFS"].split() + v["CHOLMOD_DEFS"].split() + \
        ["-I" + os.path.join(ROOT, "include")] + v["INC"].split() + \
        [os.path.join(ROOT, "tests", "schur_covariance_pairs_header_driver.cpp"), "-o", str(exe)] + libs + ["-lrt", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:] + r.stderr[-4000:]
