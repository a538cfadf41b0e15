"""The covariance parts of the Schur class of the header binding (include/slam/LinearSolver_HIP.h: CLinearSolver_Schur_HIP's
Marginals with an EBlockMatrixPart, Marginal_Columns) compile against the reference's headers, with the include paths and defines oracle/Makefile.ref
builds the drop-in driver with, and -- linked with the reference's block matrix that build() compiles into oracle/_ref
and with stand-ins for the C ABI (tests/capi_standins.h) -- write every requested part into the result.
Skip where the reference's sources (or the archives built from them) are not present."""
from header_util import run_covariance_driver, syntax_check

TU = r"""
#include "slam/LinearSolver_HIP.h"
bool covariance_parts(CLinearSolver_Schur_HIP<> &r_solver, CUberBlockMatrix &r_marginals, const CUberBlockMatrix &r_lambda)
{
	Eigen::MatrixXd columns;
	std::vector<size_t> block_columns(1, r_lambda.n_BlockColumn_Num() - 1);
	return r_solver.Marginals(r_marginals, r_lambda, EBlockMatrixPart(mpart_LastColumn | mpart_Diagonal)) &&
		r_solver.Marginals(r_marginals, r_lambda, mpart_FullMatrix, true) &&
		r_solver.Marginal_Columns(columns, r_lambda, block_columns);
}
"""


def test_schur_covariance_overloads_compile(tmp_path):
    syntax_check(tmp_path, "schur_covariance_tu.cpp", TU)


def test_schur_covariance_parts_are_written(tmp_path_factory):
    """Every part of the Marginals overload and Marginal_Columns, run on the CPU against stand-ins for the C ABI that answer
    with a known symmetric matrix, for a BA lambda with the cameras first, one the class reorders and one without a landmark
    part (its sparse solver answers): the driver checks the set of blocks written and their values."""
    run_covariance_driver(tmp_path_factory, "schur", "parts")
