// half_solves_header_driver.cpp -- runs Solve_L_Columns and Solve_Lt_Columns of both solver classes of
// include/slam/LinearSolver_HIP.h on the CPU against the stand-ins for the C ABI of tests/capi_standins.h and a stand-in
// slampp_hip_solve_half_columns of its own, which records what it is handed: each member must hand its matrix over (column-major,
// leading dimension rows()) in ONE call with its own n_half -- the caller's matrix itself where the library's order is lambda's
// own --, return false, with the library's message and the caller's matrix untouched, where the library refuses (no kept factor:
// SLAMPP_HIP_ERR_INVALID; Schur mode: SLAMPP_HIP_ERR_UNSUPPORTED), and throw on the other failure statuses.  The side of a call
// that is in the caller's order must reach the library in the library's order (the guided ordering of the Schur class: the case
// of a handle whose analysis went to the sparse path): the forward half's input holds b(r, c) = r + 1000 c + 0.5 of lambda's row r,
// which the stand-in looks for at the library's row of r, and it answers y(s, c) = 5000 + s + 0.25 c at its own row s, which must
// come back unpermuted; the backward half's input holds y(s, c) = s + 1000 c + 0.5, which must arrive unpermuted, and the
// stand-in answers x = -r - 7 - 1000 c at the library's row of lambda's row r, which the driver looks for at lambda's row r.
// Built and run by tests/test_half_solves_header.py against the reference's block matrix.  Prints "ok" and exits 0.
#include "capi_standins.h"

static int g_n_calls = 0, g_n_last_half = -1, g_n_last_columns = 0, g_n_misplaced = 0;
static int64_t g_n_last_ld = 0;
static const double *g_p_last = 0;
static int g_n_result = SLAMPP_HIP_OK;

extern "C" int slampp_hip_solve_half_columns(slampp_hip_solver *p, int n_half, double *p_inout, int64_t n_ld, int n_columns)
{
	++ g_n_calls;
	g_n_last_half = n_half;
	g_p_last = p_inout;
	g_n_last_ld = n_ld;
	g_n_last_columns = n_columns;
	if(!p || !p_inout || n_columns < 1 || n_columns > SLAMPP_HIP_SOLVE_MAX_COLUMNS || n_ld != p->cumsum.back())
		return SLAMPP_HIP_ERR_INVALID;
	if(g_n_result != SLAMPP_HIP_OK)
		return g_n_result;
	for(int c = 0; c < n_columns; ++ c) {
		for(int64_t s = 0; s < n_ld; ++ s) {
			double &r_f = p_inout[s + int64_t(c) * n_ld];
			const int64_t r = g_lambda_scalar.empty()? s : g_lambda_scalar[size_t(s)]; // lambda's row of the library's row s
			if(n_half == SLAMPP_HIP_HALF_FORWARD) {
				g_n_misplaced += r_f != double(r) + 1000.0 * c + 0.5; // b in the library's order
				r_f = 5000.0 + double(s) + 0.25 * c; // y, in the factor's order: goes back as it is
			} else {
				g_n_misplaced += r_f != double(s) + 1000.0 * c + 0.5; // y as the caller gave it
				r_f = -double(r) - 7 - 1000.0 * c; // x of lambda's row r, at the library's row
			}
		}
	}
	return SLAMPP_HIP_OK;
}

template <class CSolver>
static bool Call(CSolver &r_solver, int n_half, Eigen::MatrixXd &r_columns)
{
	return (n_half == SLAMPP_HIP_HALF_FORWARD)? r_solver.Solve_L_Columns(r_columns) : r_solver.Solve_Lt_Columns(r_columns);
}

template <class CSolver>
static void Check_Halves(const char *p_s_name, const char *p_s_dims, const size_t (*p_blocks)[2], size_t n_block_num, bool b_guided,
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
	Eigen::MatrixXd columns(n_rows, n_column_num);
	g_n_result = SLAMPP_HIP_OK;
	for(int n_half = 0; n_half < 2; ++ n_half) { // before any analysis: std::runtime_error, and the library is not called
		const int n_calls = g_n_calls;
		bool b_thrown = false;
		try {
			Call(solver, n_half, columns);
		} catch(std::runtime_error&) {
			b_thrown = true;
		}
		CHECK(b_thrown && g_n_calls == n_calls);
	}
	bool b_ok = false;
	try {
		b_ok = solver.SymbolicDecomposition_Blocky(lambda);
	} catch(std::exception &r_exc) {
		fprintf(stderr, "%s: SymbolicDecomposition_Blocky: %s\n", p_s_name, r_exc.what());
	}
	CHECK(b_ok);
	for(int n_half = 0; n_half < 2; ++ n_half) {
		for(int c = 0; c < n_column_num; ++ c)
			for(int r = 0; r < n_rows; ++ r)
				columns(r, c) = double(r) + 1000.0 * c + 0.5;
		// the call itself: the caller's matrix, once, with this member's n_half
		int n_calls = g_n_calls;
		const int n_misplaced = g_n_misplaced;
		g_n_result = SLAMPP_HIP_OK;
		b_ok = false;
		try {
			b_ok = Call(solver, n_half, columns);
		} catch(std::exception &r_exc) {
			fprintf(stderr, "%s: half %d: %s\n", p_s_name, n_half, r_exc.what());
		}
		CHECK(b_ok && solver.r_s_Half_Solve_Refusal().empty());
		CHECK(g_n_calls == n_calls + 1 && g_n_last_half == n_half && g_n_misplaced == n_misplaced);
		CHECK(!g_lambda_scalar.empty() || g_p_last == columns.data()); // (lambda's own order: the caller's matrix itself, no copy)
		CHECK(g_n_last_ld == n_rows && g_n_last_columns == n_column_num);
		int n_wrong = 0;
		for(int c = 0; c < n_column_num; ++ c)
			for(int r = 0; r < n_rows; ++ r)
				n_wrong += columns(r, c) != ((n_half == SLAMPP_HIP_HALF_FORWARD)? 5000.0 + r + 0.25 * c : -double(r) - 7 - 1000.0 * c);
		CHECK(n_wrong == 0);
		for(int c = 0; c < n_column_num; ++ c) // (the input of the cases below)
			for(int r = 0; r < n_rows; ++ r)
				columns(r, c) = double(r) + 1000.0 * c + 0.5;
		// columns of another dimension, too many columns: std::runtime_error before the library is called; none: nothing to do
		Eigen::MatrixXd columns_short(n_rows - 1, 2), columns_many(n_rows, SLAMPP_HIP_SOLVE_MAX_COLUMNS + 1), columns_none(n_rows, 0);
		columns_short.setZero();
		columns_many.setZero();
		n_calls = g_n_calls;
		for(int n_case = 0; n_case < 2; ++ n_case) {
			bool b_thrown = false;
			try {
				Call(solver, n_half, n_case? columns_many : columns_short);
			} catch(std::runtime_error&) {
				b_thrown = true;
			}
			CHECK(b_thrown && g_n_calls == n_calls);
		}
		CHECK(Call(solver, n_half, columns_none) && g_n_calls == n_calls);
		// the library refuses: false, with its message (no kept factor is SLAMPP_HIP_ERR_INVALID, Schur mode SLAMPP_HIP_ERR_UNSUPPORTED)
		const int p_refusals[] = {SLAMPP_HIP_ERR_INVALID, SLAMPP_HIP_ERR_UNSUPPORTED};
		for(int n_case = 0; n_case < 2; ++ n_case) {
			g_n_result = p_refusals[n_case];
			b_ok = true;
			bool b_thrown = false;
			try {
				b_ok = Call(solver, n_half, columns);
			} catch(std::exception&) {
				b_thrown = true;
			}
			CHECK(!b_ok && !b_thrown && solver.r_s_Half_Solve_Refusal() == "stand-in" && g_n_last_half == n_half);
			int n_touched = 0;
			for(int c = 0; c < n_column_num; ++ c)
				for(int r = 0; r < n_rows; ++ r)
					n_touched += columns(r, c) != double(r) + 1000.0 * c + 0.5;
			CHECK(n_touched == 0);
		}
		// a device error: std::runtime_error; no memory: std::bad_alloc
		g_n_result = SLAMPP_HIP_ERR_DEVICE;
		bool b_thrown = false;
		try {
			Call(solver, n_half, columns);
		} catch(std::runtime_error&) {
			b_thrown = true;
		}
		CHECK(b_thrown);
		g_n_result = SLAMPP_HIP_ERR_ALLOC;
		b_thrown = false;
		try {
			Call(solver, n_half, columns);
		} catch(std::bad_alloc&) {
			b_thrown = true;
		}
		CHECK(b_thrown);
		g_n_result = SLAMPP_HIP_OK;
	}
}

// the systems of tests/covariance_header_driver.cpp
static const size_t cameras_first[][2] = {{0, 1}, {1, 2}, {0, 3}, {1, 3}, {1, 4}, {2, 4}, {0, 5}, {2, 5}, {2, 6}};
static const size_t interleaved[][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 5}, {0, 4}, {4, 5}, {5, 6}, {0, 2}, {2, 5}};
static const size_t chain[][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {0, 3}};
static const size_t mixed[][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}, {0, 3}, {2, 5}};

int main()
{
	Check_Halves<CLinearSolver_HIP>("sparse, mixed block sizes", "323323", mixed, 7, false, 3);
	Check_Halves<CLinearSolver_HIP>("sparse, chain, one column", "66666", chain, 5, false, 1);
	Check_Halves<CLinearSolver_HIP>("sparse, chain, the most columns", "66666", chain, 5, false, SLAMPP_HIP_SOLVE_MAX_COLUMNS);
	Check_Halves<CLinearSolver_Schur_HIP<> >("schur, cameras first", "6663333", cameras_first, 9, true, 5); // (the stand-in does not know modes: the real library refuses)
	Check_Halves<CLinearSolver_Schur_HIP<> >("schur, interleaved", "6363363", interleaved, 9, true, 5); // reordered: what a handle that took the sparse path is handed
	Check_Halves<CLinearSolver_Schur_HIP<> >("schur, interleaved, the most columns", "6363363", interleaved, 9, true, SLAMPP_HIP_SOLVE_MAX_COLUMNS);
	Check_Halves<CLinearSolver_Schur_HIP<> >("schur, no landmark part", "66666", chain, 5, false, 4); // the class's sparse solver answers
	if(n_failures) {
		fprintf(stderr, "%d failures\n", n_failures);
		return 1;
	}
	printf("ok\n");
	return 0;
}
