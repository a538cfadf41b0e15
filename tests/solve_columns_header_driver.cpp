// solve_columns_header_driver.cpp -- runs Solve_Again_Columns of both solver classes of include/slam/LinearSolver_HIP.h on the
// CPU against the stand-ins for the C ABI of tests/capi_standins.h and a stand-in slampp_hip_solve_columns of its own.  The
// caller's matrix holds eta(r, c) = r + 1000 c + 0.5, so the stand-in can tell whether every entry it is handed sits at the row
// the library's order gives it (the guided ordering, cameras first, for the Schur class), with the leading dimension rows() and
// at most SLAMPP_HIP_SOLVE_MAX_COLUMNS columns a call; where the library's order is lambda's own it must be handed the
// caller's matrix itself (one host call, no copy).  It answers -value - 7 in place, which the driver finds at the caller's
// rows.  Built and run by tests/test_solve_columns_header.py against the reference's block matrix.  Prints "ok" and exits 0.
#include "capi_standins.h"

static int g_n_calls = 0, g_n_misplaced = 0, g_n_bad_args = 0, g_n_columns_seen = 0;
static int g_n_result = SLAMPP_HIP_OK;
static const double *g_p_expected = 0; // where the caller's matrix begins, if it must be handed over as it is
static int64_t g_n_expected_rows = 0;

static double f_Eta(int64_t r, int64_t c) { return double(r) + 1000.0 * double(c) + 0.5; }

extern "C" int slampp_hip_solve_columns(slampp_hip_solver *p, double *p_rhs_inout, int64_t n_ld, int n_columns)
{
	++ g_n_calls;
	if(!p || !p_rhs_inout || n_columns < 1 || n_columns > SLAMPP_HIP_SOLVE_MAX_COLUMNS || n_ld != g_n_expected_rows ||
	   n_ld != p->cumsum.back()) {
		++ g_n_bad_args;
		return SLAMPP_HIP_ERR_INVALID;
	}
	if(g_n_result != SLAMPP_HIP_OK)
		return g_n_result;
	if(g_p_expected && p_rhs_inout != g_p_expected + int64_t(g_n_columns_seen) * n_ld)
		++ g_n_bad_args; // (a copy where none is needed, or the groups out of order)
	for(int c = 0; c < n_columns; ++ c) {
		for(int64_t s = 0; s < n_ld; ++ s) {
			double &r_f = p_rhs_inout[s + int64_t(c) * n_ld];
			const int64_t r = g_lambda_scalar.empty()? s : g_lambda_scalar[size_t(s)];
			if(r_f != f_Eta(r, g_n_columns_seen + c))
				++ g_n_misplaced;
			r_f = -r_f - 7;
		}
	}
	g_n_columns_seen += n_columns;
	return SLAMPP_HIP_OK;
}

template <class CSolver>
static void Check_Columns(const char *p_s_name, const char *p_s_dims, const size_t (*p_blocks)[2], size_t n_block_num, bool b_guided,
	int n_column_num)
{
	std::vector<size_t> dims;
	for(; *p_s_dims; ++ p_s_dims)
		dims.push_back(size_t(*p_s_dims - '0'));
	TBlockSet blocks;
	for(size_t c = 0; c < dims.size(); ++ c)
		blocks.insert(std::make_pair(c, c));
	for(size_t k = 0; k < n_block_num; ++ k)
		blocks.insert(std::make_pair(p_blocks[k][0], p_blocks[k][1]));
	CUberBlockMatrix lambda;
	Make_Lambda(lambda, dims, blocks);
	Set_Library_Order(lambda, dims, b_guided);
	const int n_rows = int(lambda.n_Column_Num());
	CSolver solver;
	Eigen::MatrixXd eta(n_rows, n_column_num);
	for(int c = 0; c < n_column_num; ++ c)
		for(int r = 0; r < n_rows; ++ r)
			eta(r, c) = f_Eta(r, c);
	g_n_result = SLAMPP_HIP_OK;
	g_n_expected_rows = n_rows;
	// before any analysis: std::runtime_error, and the library is not called
	int n_calls = g_n_calls;
	bool b_thrown = false;
	try {
		solver.Solve_Again_Columns(eta);
	} catch(std::runtime_error&) {
		b_thrown = true;
	}
	CHECK(b_thrown && g_n_calls == n_calls);
	bool b_ok = false;
	try {
		b_ok = solver.SymbolicDecomposition_Blocky(lambda);
	} catch(std::exception &r_exc) {
		fprintf(stderr, "%s: SymbolicDecomposition_Blocky: %s\n", p_s_name, r_exc.what());
	}
	CHECK(b_ok);
	// the call itself: every entry where the library's order has it, the answers back at the caller's rows
	const int n_misplaced = g_n_misplaced, n_bad_args = g_n_bad_args;
	n_calls = g_n_calls;
	g_n_columns_seen = 0;
	g_p_expected = g_lambda_scalar.empty()? &eta(0, 0) : 0;
	b_ok = false;
	try {
		b_ok = solver.Solve_Again_Columns(eta);
	} catch(std::exception &r_exc) {
		fprintf(stderr, "%s: Solve_Again_Columns: %s\n", p_s_name, r_exc.what());
	}
	CHECK(b_ok);
	CHECK(g_n_calls == n_calls + (n_column_num + SLAMPP_HIP_SOLVE_MAX_COLUMNS - 1) / SLAMPP_HIP_SOLVE_MAX_COLUMNS); // one host call per 256 columns
	CHECK(g_n_columns_seen == n_column_num);
	CHECK(g_n_misplaced == n_misplaced && g_n_bad_args == n_bad_args);
	int n_wrong = 0;
	for(int c = 0; c < n_column_num; ++ c)
		for(int r = 0; r < n_rows; ++ r)
			n_wrong += eta(r, c) != -f_Eta(r, c) - 7;
	CHECK(n_wrong == 0);
	g_p_expected = 0;
	// right-hand sides of another dimension: std::runtime_error before the library is called
	Eigen::MatrixXd eta_short(n_rows - 1, 2);
	eta_short.setZero();
	n_calls = g_n_calls;
	b_thrown = false;
	try {
		solver.Solve_Again_Columns(eta_short);
	} catch(std::runtime_error&) {
		b_thrown = true;
	}
	CHECK(b_thrown && g_n_calls == n_calls);
	// no columns: nothing to do
	Eigen::MatrixXd eta_none(n_rows, 0);
	CHECK(solver.Solve_Again_Columns(eta_none) && g_n_calls == n_calls);
	// any failure status: std::runtime_error (no kept factor is SLAMPP_HIP_ERR_INVALID); no memory: std::bad_alloc
	g_n_columns_seen = 0;
	g_n_result = SLAMPP_HIP_ERR_INVALID;
	b_thrown = false;
	try {
		solver.Solve_Again_Columns(eta);
	} catch(std::runtime_error&) {
		b_thrown = true;
	}
	CHECK(b_thrown);
	g_n_result = SLAMPP_HIP_ERR_ALLOC;
	b_thrown = false;
	try {
		solver.Solve_Again_Columns(eta);
	} catch(std::bad_alloc&) {
		b_thrown = true;
	}
	CHECK(b_thrown);
	g_n_result = SLAMPP_HIP_OK;
}

// the systems of tests/covariance_header_driver.cpp
static const size_t cameras_first[][2] = {{0, 1}, {1, 2}, {0, 3}, {1, 3}, {1, 4}, {2, 4}, {0, 5}, {2, 5}, {2, 6}};
static const size_t interleaved[][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 5}, {0, 4}, {4, 5}, {5, 6}, {0, 2}, {2, 5}};
static const size_t chain[][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {0, 3}};
static const size_t mixed[][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}, {0, 3}, {2, 5}};

int main()
{
	Check_Columns<CLinearSolver_HIP>("sparse, mixed block sizes", "323323", mixed, 7, false, 3);
	Check_Columns<CLinearSolver_HIP>("sparse, chain, one column", "66666", chain, 5, false, 1);
	Check_Columns<CLinearSolver_HIP>("sparse, chain, two host calls", "66666", chain, 5, false, SLAMPP_HIP_SOLVE_MAX_COLUMNS + 44);
	Check_Columns<CLinearSolver_Schur_HIP<> >("schur, cameras first", "6663333", cameras_first, 9, true, 5);
	Check_Columns<CLinearSolver_Schur_HIP<> >("schur, interleaved", "6363363", interleaved, 9, true, 5); // reordered: the rows are permuted by blocks
	Check_Columns<CLinearSolver_Schur_HIP<> >("schur, interleaved, two host calls", "6363363", interleaved, 9, true, SLAMPP_HIP_SOLVE_MAX_COLUMNS + 1);
	Check_Columns<CLinearSolver_Schur_HIP<> >("schur, no landmark part", "66666", chain, 5, false, 4); // the class's sparse solver answers
	if(n_failures) {
		fprintf(stderr, "%d failures\n", n_failures);
		return 1;
	}
	printf("ok\n");
	return 0;
}
