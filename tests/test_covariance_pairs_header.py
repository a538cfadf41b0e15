"""The pair parts of the header binding (include/slam/LinearSolver_HIP.h: Marginal_Blocks, Joint_Marginal) compile
against the reference's headers, with the include paths and defines oracle/Makefile.ref builds the drop-in driver with.
Skipped where the reference's headers are not present."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TU = r"""
#include "slam/LinearSolver_HIP.h"
bool covariance_pairs(CLinearSolver_HIP &r_solver, const CUberBlockMatrix &r_lambda)
{
	const size_t n_last = r_lambda.n_BlockColumn_Num() - 1;
	std::vector<std::pair<size_t, size_t> > pairs;
	pairs.push_back(std::make_pair(size_t(0), n_last));
	pairs.push_back(std::make_pair(n_last, size_t(0)));
	pairs.push_back(std::make_pair(n_last, n_last));
	std::vector<Eigen::MatrixXd> blocks;
	std::vector<size_t> block_columns(1, n_last);
	block_columns.push_back(0);
	Eigen::MatrixXd joint;
	return r_solver.Marginal_Blocks(blocks, r_lambda, pairs) && r_solver.Joint_Marginal(joint, r_lambda, block_columns) &&
		blocks.size() == 3 && joint.rows() == joint.cols();
}
"""


def _makefile_vars():
    text = open(os.path.join(ROOT, "oracle", "Makefile.ref")).read()
    out = {}
    for name in ("REF", "OUT", "OPT", "CDEFS", "INC", "CHOLMOD_DEFS"):
        m = re.search(r"^%s\s*[?:]?=\s*(.*)$" % name, text, re.M)
        assert m, name
        out[name] = m.group(1).strip()
    for name in ("OPT", "CDEFS", "INC", "CHOLMOD_DEFS"):
        out[name] = out[name].replace("$(REF)", out["REF"]).replace("$(OUT)", os.path.join(ROOT, out["OUT"]))
    return out


def test_header_declares_the_pair_members():
    """(runs everywhere: the members and the C entry they call are there)"""
    text = open(os.path.join(ROOT, "include", "slam", "LinearSolver_HIP.h")).read()
    assert re.search(r"bool\s+Marginal_Blocks\s*\(\s*std::vector<Eigen::MatrixXd>\s*&", text)
    assert re.search(r"bool\s+Joint_Marginal\s*\(\s*Eigen::MatrixXd\s*&", text)
    capi = open(os.path.join(ROOT, "include", "slampp_hip.h")).read()
    assert "slampp_hip_marginal_blocks(" in capi and "slampp_hip_marginal_blocks_device_async(" in capi


def test_pair_members_compile(tmp_path):
    v = _makefile_vars()
    if not os.path.isdir(os.path.join(v["REF"], "include", "slam")):
        pytest.skip("the reference's headers are not present")
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = tmp_path / "covariance_pairs_tu.cpp"
    src.write_text(TU)
    cmd = ["g++", "-fsyntax-only", "-w"] + v["OPT"].split() + v["CDEFS"].split() + v["CHOLMOD_DEFS"].split() + \
        ["-I" + os.path.join(ROOT, "include")] + v["INC"].split() + [str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
