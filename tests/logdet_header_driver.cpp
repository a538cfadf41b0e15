// logdet_header_driver.cpp -- runs Log_Determinant of both solver classes of include/slam/LinearSolver_HIP.h (and of the
// CLinearSolver_Schur<CLinearSolver_HIP, ..> specialization's base) on the CPU against the stand-ins for the C ABI of
// tests/capi_standins.h and a stand-in slampp_hip_logdet of its own.  Lambda's scalar (i, j) holds S(i, j) of the stand-ins, so the
// stand-in can tell whether every value it is handed sits where the structure it was given says -- in the library's order:
// the guided ordering (cameras first) for the Schur class, with the blocks that land below the diagonal transposed -- and
// answers with a known function of the values: the sum of (1 + position mod 7) * value.  Built and run by
// tests/test_logdet_header.py against the reference's block matrix.  Prints "ok" and exits 0.
#include "capi_standins.h"

static int g_n_logdet_calls = 0, g_n_logdet_misplaced = 0, g_n_logdet_reuse = 0;
static int g_n_logdet_result = SLAMPP_HIP_OK;
static double g_f_logdet_answer = 0; // what the last call answered

extern "C" int slampp_hip_logdet(slampp_hip_solver *p, const double *p_values, int b_reuse_factor, double *p_logdet)
{
	++ g_n_logdet_calls;
	g_n_logdet_reuse += b_reuse_factor != 0;
	if(!p || !p_values || !p_logdet)
		return SLAMPP_HIP_ERR_INVALID;
	*p_logdet = std::nan("");
	if(g_n_logdet_result != SLAMPP_HIP_OK)
		return g_n_logdet_result;
	double f_sum = 0;
	size_t k = 0;
	for(size_t c = 0; c + 1 < p->cumsum.size(); ++ c) {
		for(int64_t b = p->bcol_ptr[c]; b < p->bcol_ptr[c + 1]; ++ b) {
			const int64_t R = p->brow[size_t(b)], dr = p->cumsum[size_t(R) + 1] - p->cumsum[size_t(R)], dc = p->cumsum[c + 1] - p->cumsum[c];
			for(int64_t q = 0; q < dc; ++ q) {
				for(int64_t r = 0; r < dr; ++ r, ++ k) {
					if(p_values[k] != S_lib(p->cumsum[size_t(R)] + r, p->cumsum[c] + q))
						++ g_n_logdet_misplaced;
					f_sum += double(1 + k % 7) * p_values[k];
				}
			}
		}
	}
	if(k != p->values.size())
		++ g_n_logdet_misplaced;
	*p_logdet = g_f_logdet_answer = f_sum;
	return SLAMPP_HIP_OK;
}

// lambda with the given upper blocks, scalar (i, j) = S(i, j)
static void Make_S_Lambda(CUberBlockMatrix &r_lambda, const std::vector<size_t> &r_dims, const TBlockSet &r_blocks)
{
	Make_Lambda(r_lambda, r_dims, r_blocks);
	for(TBlockSet::const_iterator p_it = r_blocks.begin(); p_it != r_blocks.end(); ++ p_it) {
		const size_t r = p_it->first, c = p_it->second;
		double *p = r_lambda.p_GetBlock_Log(r, c, r_dims[r], r_dims[c], true, false);
		CHECK(p != 0);
		const size_t r0 = r_lambda.n_BlockColumn_Base(r), c0 = r_lambda.n_BlockColumn_Base(c);
		for(size_t q = 0; p && q < r_dims[c]; ++ q)
			for(size_t a = 0; a < r_dims[r]; ++ a)
				p[a + q * r_dims[r]] = S(int64_t(r0 + a), int64_t(c0 + q));
	}
}

template <class CSolver>
static void Check_Logdet(const char *p_s_name, const char *p_s_dims, const size_t (*p_blocks)[2], size_t n_block_num, bool b_guided)
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
	Make_S_Lambda(lambda, dims, blocks);
	Set_Library_Order(lambda, dims, b_guided);
	CSolver solver;
	g_n_logdet_result = SLAMPP_HIP_OK;
	const int n_calls = g_n_logdet_calls, n_misplaced = g_n_logdet_misplaced, n_reuse = g_n_logdet_reuse;
	double f_logdet = -1;
	bool b_ok = false;
	try {
		b_ok = solver.Log_Determinant(f_logdet, lambda);
	} catch(std::exception &r_exc) {
		fprintf(stderr, "%s: Log_Determinant: %s\n", p_s_name, r_exc.what());
	}
	CHECK(b_ok);
	CHECK(g_n_logdet_calls == n_calls + 1);
	CHECK(g_n_logdet_reuse == n_reuse); // b_reuse_factor = 0: the values are factored
	CHECK(g_n_logdet_misplaced == n_misplaced); // every value where the library's order has it
	CHECK(f_logdet == g_f_logdet_answer && f_logdet > 0); // the result passes through
	// a second call on the same lambda: the cached analysis, the same answer
	double f_again = -1;
	CHECK(solver.Log_Determinant(f_again, lambda) && f_again == f_logdet && g_n_logdet_misplaced == n_misplaced);
	// not positive definite: false, no exception
	g_n_logdet_result = SLAMPP_HIP_NOT_POSDEF;
	bool b_thrown = false;
	b_ok = true;
	try {
		b_ok = solver.Log_Determinant(f_logdet, lambda);
	} catch(std::exception&) {
		b_thrown = true;
	}
	CHECK(!b_ok && !b_thrown && f_logdet != f_logdet); // (NaN is what the library leaves)
	// any other status: std::runtime_error; no memory: std::bad_alloc
	g_n_logdet_result = SLAMPP_HIP_ERR_UNSUPPORTED;
	b_thrown = false;
	try {
		solver.Log_Determinant(f_logdet, lambda);
	} catch(std::runtime_error&) {
		b_thrown = true;
	}
	CHECK(b_thrown);
	g_n_logdet_result = SLAMPP_HIP_ERR_ALLOC;
	b_thrown = false;
	try {
		solver.Log_Determinant(f_logdet, lambda);
	} catch(std::bad_alloc&) {
		b_thrown = true;
	}
	CHECK(b_thrown);
	g_n_logdet_result = SLAMPP_HIP_OK;
}

// the systems of tests/covariance_header_driver.cpp
static const size_t cameras_first[][2] = {{0, 1}, {1, 2}, {0, 3}, {1, 3}, {1, 4}, {2, 4}, {0, 5}, {2, 5}, {2, 6}};
static const size_t interleaved[][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 5}, {0, 4}, {4, 5}, {5, 6}, {0, 2}, {2, 5}};
static const size_t chain[][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {0, 3}};
static const size_t mixed[][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}, {0, 3}, {2, 5}};

int main()
{
	Check_Logdet<CLinearSolver_HIP>("sparse, mixed block sizes", "323323", mixed, 7, false);
	Check_Logdet<CLinearSolver_HIP>("sparse, chain", "66666", chain, 5, false);
	Check_Logdet<CLinearSolver_Schur_HIP<> >("schur, cameras first", "6663333", cameras_first, 9, true);
	Check_Logdet<CLinearSolver_Schur_HIP<> >("schur, interleaved", "6363363", interleaved, 9, true); // reordered: some blocks arrive transposed
	Check_Logdet<CLinearSolver_Schur_HIP<> >("schur, no landmark part", "66666", chain, 5, false); // the class's sparse solver answers
	if(n_failures) {
		fprintf(stderr, "%d failures\n", n_failures);
		return 1;
	}
	printf("ok\n");
	return 0;
}
