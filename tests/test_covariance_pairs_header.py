"""The pair parts of the header binding (include/slam/LinearSolver_HIP.h: Marginal_Blocks, Joint_Marginal) compile
against the reference's headers, with the include paths and defines oracle/Makefile.ref builds the drop-in driver with,
and -- linked with the reference's block matrix that build() compiles into oracle/_ref and with stand-ins for the C ABI
(tests/capi_standins.h) -- return block (r, c) of lambda for every pair.
Skip where the reference's sources (or the archives built from them) are not present."""
import os
import re

from header_util import ROOT, run_covariance_driver, syntax_check

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


def test_header_declares_the_pair_members():
    """(runs everywhere: the members and the C entry they call are there)"""
    text = open(os.path.join(ROOT, "include", "slam", "LinearSolver_HIP.h")).read()
    assert re.search(r"bool\s+Marginal_Blocks\s*\(\s*std::vector<Eigen::MatrixXd>\s*&", text)
    assert re.search(r"bool\s+Joint_Marginal\s*\(\s*Eigen::MatrixXd\s*&", text)
    capi = open(os.path.join(ROOT, "include", "slampp_hip.h")).read()
    assert "slampp_hip_marginal_blocks(" in capi and "slampp_hip_marginal_blocks_device_async(" in capi


def test_pair_members_compile(tmp_path):
    syntax_check(tmp_path, "covariance_pairs_tu.cpp", TU)


def test_covariance_pairs_are_the_blocks_of_lambda(tmp_path_factory):
    """Marginal_Blocks at every ordered pair -- first > second, outside lambda's pattern and one listed twice among them --
    and Joint_Marginal of a set of columns, run on the CPU against stand-ins for the C ABI that answer with a known
    symmetric matrix, for a chain of 5 block columns of width 6 with one closure; the refusals of an index out of range,
    a column listed twice and an empty set."""
    run_covariance_driver(tmp_path_factory, "sparse", "pairs")
