"""Marginal_Blocks and Joint_Marginal of the Schur class of the header binding (include/slam/LinearSolver_HIP.h:
CLinearSolver_Schur_HIP) compile against the reference's headers, with the include paths and defines oracle/Makefile.ref
builds the drop-in driver with, and -- linked with the reference's block matrix that build() compiles into oracle/_ref
and with stand-ins for the C ABI (tests/capi_standins.h) -- return block (r, c) of lambda's own
order for every pair.  Skip where the reference's sources (or the archives built from them) are not present."""
from header_util import run_covariance_driver, syntax_check

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


def test_schur_covariance_pair_members_compile(tmp_path):
    syntax_check(tmp_path, "schur_covariance_pairs_tu.cpp", TU)


def test_schur_covariance_pairs_are_the_blocks_of_lambdas_order(tmp_path_factory):
    """Marginal_Blocks at every ordered pair and Joint_Marginal of a mixed set, run on the CPU against stand-ins for the C ABI
    that answer with a known symmetric matrix, for a BA lambda with the cameras first, one the class reorders (pairs reach the
    library turned around) and one without a landmark part (its sparse solver answers)."""
    run_covariance_driver(tmp_path_factory, "schur", "pairs")
