// schur_covariance_header_driver.cpp -- runs the covariance parts of CLinearSolver_Schur_HIP (include/slam/LinearSolver_HIP.h:
// Marginals with an EBlockMatrixPart, Marginal_Columns) on the CPU against stand-ins for the C ABI.  The stand-ins answer every
// covariance request with a known symmetric matrix S(r, c) of lambda's scalars, seen through the guided ordering the class
// hands the library, so the driver checks which blocks the header writes where, and with what -- for a BA lambda with the
// cameras first, one whose cameras and landmarks are interleaved (the class reorders it), and one without a landmark part
// (the class's sparse solver answers).  Built and run by tests/test_schur_covariance_header.py against the reference's block
// matrix.  Prints "ok" and exits 0.
#include "slam/LinearSolver_HIP.h"
#include <cmath>
#include <map>
#include <set>

// ---- stand-ins for the C ABI (what the header calls) ----

struct slampp_hip_solver {
	std::vector<int64_t> cumsum, bcol_ptr;
	std::vector<int32_t> brow;
	std::vector<double> values, rhs;
};

static double S(int64_t r, int64_t c) // the "covariance": symmetric, every entry distinct (lambda's scalar indices)
{
	const int64_t a = std::min(r, c), b = std::max(r, c);
	return double(a) * 1009 + double(b) + 0.25;
}

// the library sees lambda in the Schur class's guided order: its scalar s is lambda's scalar g_lambda_scalar[s] (empty: the same)
static std::vector<int64_t> g_lambda_scalar;
static int g_n_schur_calls = 0; // calls of the Schur covariance stand-ins

static double S_lib(int64_t r, int64_t c) // the covariance at the library's scalars (r, c)
{
	return (g_lambda_scalar.empty())? S(r, c) : S(g_lambda_scalar[size_t(r)], g_lambda_scalar[size_t(c)]);
}

extern "C" {
int slampp_hip_create(slampp_hip_solver **pp, int) { *pp = new slampp_hip_solver(); return SLAMPP_HIP_OK; }
int slampp_hip_create_multi(slampp_hip_solver **pp, const int *, int) { *pp = new slampp_hip_solver(); return SLAMPP_HIP_OK; }
int slampp_hip_group_info(const slampp_hip_solver *, int *p_n, int64_t *, int, const char **) { if(p_n) *p_n = 0; return SLAMPP_HIP_OK; }
void slampp_hip_destroy(slampp_hip_solver *p) { delete p; }
const char *slampp_hip_last_error(const slampp_hip_solver *) { return "stand-in"; }
int slampp_hip_set_option(slampp_hip_solver *, const char *, int64_t) { return SLAMPP_HIP_OK; }
int slampp_hip_set_structure(slampp_hip_solver *p, int64_t n, const int64_t *cs, const int64_t *ptr, const int32_t *brow)
{
	p->cumsum.assign(cs, cs + n + 1);
	p->bcol_ptr.assign(ptr, ptr + n + 1);
	p->brow.assign(brow, brow + ptr[n]);
	int64_t n_values = 0;
	for(int64_t c = 0; c < n; ++ c) {
		for(int64_t b = ptr[c]; b < ptr[c + 1]; ++ b)
			n_values += (cs[brow[b] + 1] - cs[brow[b]]) * (cs[c + 1] - cs[c]);
	}
	p->values.assign(size_t(n_values), 0.0);
	p->rhs.assign(size_t(cs[n]), 0.0);
	return SLAMPP_HIP_OK;
}
int slampp_hip_analyze(slampp_hip_solver *, int, int64_t) { return SLAMPP_HIP_OK; }
int slampp_hip_host_staging(slampp_hip_solver *p, double **pv, double **pr) { *pv = &p->values[0]; *pr = &p->rhs[0]; return SLAMPP_HIP_OK; }
int slampp_hip_upload_values_async(slampp_hip_solver *, int64_t, int64_t) { return SLAMPP_HIP_OK; }
int slampp_hip_factor_solve(slampp_hip_solver *, const double *, double *, slampp_hip_times *) { return SLAMPP_HIP_ERR_UNSUPPORTED; }
int slampp_hip_solve_marginal_poses(slampp_hip_solver *, const double *, double *) { return SLAMPP_HIP_ERR_UNSUPPORTED; }
int slampp_hip_factorize(slampp_hip_solver *, const double *, double *) { return SLAMPP_HIP_ERR_UNSUPPORTED; }
int slampp_hip_factor_structure(const slampp_hip_solver *, int64_t *, int64_t *, int64_t *, int32_t *, int32_t *, int64_t *, int32_t *,
	int64_t *) { return SLAMPP_HIP_ERR_UNSUPPORTED; }
int slampp_hip_schur_set_changed_points(slampp_hip_solver *, const int64_t *, int64_t) { return SLAMPP_HIP_ERR_UNSUPPORTED; }
int slampp_hip_schur_marginals(slampp_hip_solver *, const double *, double *, double *) { return SLAMPP_HIP_ERR_UNSUPPORTED; }
int slampp_hip_marginals(slampp_hip_solver *p, const double *, double *out)
{
	for(size_t c = 0; c + 1 < p->cumsum.size(); ++ c) {
		const int64_t d = p->cumsum[c + 1] - p->cumsum[c];
		for(int64_t q = 0; q < d; ++ q)
			for(int64_t r = 0; r < d; ++ r)
				*out ++ = S_lib(p->cumsum[c] + r, p->cumsum[c] + q);
	}
	return SLAMPP_HIP_OK;
}
int slampp_hip_marginals_pattern(slampp_hip_solver *p, const double *, double *out)
{
	for(size_t c = 0; c + 1 < p->cumsum.size(); ++ c) {
		for(int64_t b = p->bcol_ptr[c]; b < p->bcol_ptr[c + 1]; ++ b) {
			const int64_t R = p->brow[size_t(b)], dr = p->cumsum[R + 1] - p->cumsum[R], dc = p->cumsum[c + 1] - p->cumsum[c];
			for(int64_t q = 0; q < dc; ++ q)
				for(int64_t r = 0; r < dr; ++ r)
					*out ++ = S_lib(p->cumsum[R] + r, p->cumsum[c] + q);
		}
	}
	return SLAMPP_HIP_OK;
}
int slampp_hip_marginal_columns(slampp_hip_solver *p, const double *, int n_cols, const int64_t *bcols, double *out)
{
	const int64_t n = p->cumsum.back();
	for(int i = 0; i < n_cols; ++ i) {
		for(int64_t s = p->cumsum[size_t(bcols[i])]; s < p->cumsum[size_t(bcols[i]) + 1]; ++ s)
			for(int64_t r = 0; r < n; ++ r)
				*out ++ = S_lib(r, s);
	}
	return SLAMPP_HIP_OK;
}
int slampp_hip_schur_marginals_pattern(slampp_hip_solver *p, const double *, double *out)
{
	++ g_n_schur_calls;
	return slampp_hip_marginals_pattern(p, 0, out);
}
int slampp_hip_schur_marginals_pattern_device_async(slampp_hip_solver *, const double *, double *) { return SLAMPP_HIP_ERR_UNSUPPORTED; }
int slampp_hip_schur_marginal_columns(slampp_hip_solver *p, const double *, int n_cols, const int64_t *bcols, double *out)
{
	++ g_n_schur_calls;
	return slampp_hip_marginal_columns(p, 0, n_cols, bcols, out);
}
int slampp_hip_schur_marginal_columns_device_async(slampp_hip_solver *, const double *, int, const int64_t *, double *) { return SLAMPP_HIP_ERR_UNSUPPORTED; }
} // extern "C"

// ---- the checks ----

static int n_failures = 0;
#define CHECK(c) do { if(!(c)) { fprintf(stderr, "failed at line %d: %s\n", __LINE__, #c); ++ n_failures; } } while(0)

typedef std::set<std::pair<size_t, size_t> > TBlockSet;

// the blocks of r_m must be exactly r_expected (i, j) (upper triangle), each equal to S on its rows and columns
static void Check_Blocks(const CUberBlockMatrix &r_m, const CUberBlockMatrix &r_lambda, const TBlockSet &r_expected, const char *p_s_what)
{
	TBlockSet found;
	CHECK(r_m.n_BlockColumn_Num() == r_lambda.n_BlockColumn_Num() && r_m.n_Column_Num() == r_lambda.n_Column_Num());
	for(size_t j = 0; j < r_m.n_BlockColumn_Num(); ++ j) {
		for(size_t k = 0; k < r_m.n_BlockColumn_Block_Num(j); ++ k) {
			const size_t i = r_m.n_Block_Row(j, k);
			found.insert(std::make_pair(i, j));
			CUberBlockMatrix::_TyConstMatrixXdRef t_blk = r_m.t_Block_AtColumn(j, k);
			const size_t r0 = r_lambda.n_BlockColumn_Base(i), c0 = r_lambda.n_BlockColumn_Base(j);
			CHECK(size_t(t_blk.rows()) == r_lambda.n_BlockColumn_Column_Num(i) && size_t(t_blk.cols()) == r_lambda.n_BlockColumn_Column_Num(j));
			for(int c = 0; c < t_blk.cols(); ++ c)
				for(int r = 0; r < t_blk.rows(); ++ r)
					CHECK(t_blk(r, c) == S(int64_t(r0 + r), int64_t(c0 + c)));
		}
	}
	if(found != r_expected) {
		fprintf(stderr, "%s: %d blocks, %d expected\n", p_s_what, int(found.size()), int(r_expected.size()));
		++ n_failures;
	}
}

// lambda of the given block sizes with the given upper blocks (r <= c); a dominant diagonal
static void Make_Lambda(CUberBlockMatrix &r_lambda, const std::vector<size_t> &r_dims, const TBlockSet &r_blocks)
{
	for(size_t c = 0; c < r_dims.size(); ++ c) { // column by column: a block row exists before it is used further on
		for(size_t r = 0; r <= c; ++ r) {
			if(!r_blocks.count(std::make_pair(r, c)))
				continue;
				double *p = r_lambda.p_GetBlock_Log(r, c, r_dims[r], r_dims[c], true, false);
			CHECK(p != 0);
			for(size_t e = 0; p && e < r_dims[r] * r_dims[c]; ++ e)
				p[e] = (r == c && e % (r_dims[c] + 1) == 0)? 10.0 : 0.1;
		}
	}
}

// every part combination and Marginal_Columns on one lambda; b_schur: the Schur covariance entries must have answered
static void Check_System(const std::vector<size_t> &r_dims, const TBlockSet &r_lam_blocks, bool b_schur, const char *p_s_system)
{
	const size_t n = r_dims.size();
	CUberBlockMatrix lambda;
	Make_Lambda(lambda, r_dims, r_lam_blocks);
	// the guided ordering the class computes (the widest block columns first, then the others, both in stable order)
	const size_t n_wide = *std::max_element(r_dims.begin(), r_dims.end());
	std::vector<size_t> order;
	for(size_t i = 0; i < n; ++ i)
		if(r_dims[i] == n_wide)
			order.push_back(i);
	for(size_t i = 0; i < n; ++ i)
		if(r_dims[i] != n_wide)
			order.push_back(i);
	g_lambda_scalar.clear();
	if(b_schur) {
		for(size_t i = 0; i < n; ++ i)
			for(size_t d = 0; d < r_dims[order[i]]; ++ d)
				g_lambda_scalar.push_back(int64_t(lambda.n_BlockColumn_Base(order[i]) + d));
	}
	TBlockSet diag, last_block, last_col, full;
	for(size_t j = 0; j < n; ++ j) {
		diag.insert(std::make_pair(j, j));
		last_col.insert(std::make_pair(j, n - 1));
		for(size_t i = 0; i <= j; ++ i)
			full.insert(std::make_pair(i, j));
	}
	last_block.insert(std::make_pair(n - 1, n - 1));
	struct { int n_part; bool b_lambda; const TBlockSet *p_a, *p_b; const char *p_s_name; } cases[] = {
		{mpart_LastBlock, false, &last_block, 0, "mpart_LastBlock"},
		{mpart_LastColumn, false, &last_col, 0, "mpart_LastColumn"},
		{mpart_Diagonal, false, &diag, 0, "mpart_Diagonal"},
		{mpart_LastColumn | mpart_Diagonal, false, &last_col, &diag, "mpart_LastColumn | mpart_Diagonal"},
		{mpart_LastBlock | mpart_Diagonal, false, &last_block, &diag, "mpart_LastBlock | mpart_Diagonal"},
		{mpart_FullMatrix, false, &full, 0, "mpart_FullMatrix"},
		{mpart_FullMatrix, true, &full, 0, "mpart_FullMatrix + lambda's structure"},
		{mpart_Diagonal, true, &diag, &r_lam_blocks, "mpart_Diagonal + lambda's structure"},
		{mpart_LastBlock, true, &last_block, &r_lam_blocks, "mpart_LastBlock + lambda's structure"},
		{mpart_LastColumn, true, &last_col, &r_lam_blocks, "mpart_LastColumn + lambda's structure"},
		{mpart_Nothing, true, &r_lam_blocks, 0, "lambda's structure"}
	};
	CLinearSolver_Schur_HIP<> solver;
	for(size_t t = 0; t < sizeof(cases) / sizeof(cases[0]); ++ t) {
		TBlockSet expected(*cases[t].p_a);
		if(cases[t].p_b)
			expected.insert(cases[t].p_b->begin(), cases[t].p_b->end());
		CUberBlockMatrix marginals;
		bool b_ok = false;
		const int n_calls_before = g_n_schur_calls;
		try {
			b_ok = solver.Marginals(marginals, lambda, EBlockMatrixPart(cases[t].n_part), cases[t].b_lambda);
		} catch(std::exception &r_exc) {
			fprintf(stderr, "%s, %s: %s\n", p_s_system, cases[t].p_s_name, r_exc.what());
		}
		CHECK(b_ok);
		CHECK((g_n_schur_calls > n_calls_before) == b_schur);
		if(b_ok) {
			std::string s_name = std::string(p_s_system) + ", " + cases[t].p_s_name;
			Check_Blocks(marginals, lambda, expected, s_name.c_str());
		}
	}
	// mpart_Column does not say which column: refused, alone and in a union
	const int column_parts[] = {mpart_Column, mpart_Column | mpart_Diagonal, mpart_Column | mpart_LastColumn};
	for(size_t t = 0; t < 3; ++ t) {
		CUberBlockMatrix marginals;
		bool b_thrown = false;
		try {
			solver.Marginals(marginals, lambda, EBlockMatrixPart(column_parts[t]));
		} catch(std::runtime_error&) {
			b_thrown = true;
		}
		CHECK(b_thrown);
	}
	// Marginal_Columns: n_scalars x k, the listed columns in order, rows in lambda's scalar order
	std::vector<size_t> cols;
	cols.push_back(n - 2);
	cols.push_back(0);
	cols.push_back(1);
	Eigen::MatrixXd X;
	CHECK(solver.Marginal_Columns(X, lambda, cols));
	size_t n_k = 0;
	for(size_t q = 0; q < cols.size(); ++ q)
		n_k += r_dims[cols[q]];
	CHECK(size_t(X.rows()) == lambda.n_Column_Num() && size_t(X.cols()) == n_k);
	for(size_t q = 0, c = 0; q < cols.size() && size_t(X.cols()) == n_k; ++ q) {
		for(size_t d = 0; d < r_dims[cols[q]]; ++ d, ++ c) {
			const int64_t s = int64_t(lambda.n_BlockColumn_Base(cols[q]) + d);
			for(int r = 0; r < X.rows(); ++ r)
				CHECK(X(r, int(c)) == S(r, s));
		}
	}
	bool b_thrown = false;
	try {
		std::vector<size_t> bad(1, n);
		solver.Marginal_Columns(X, lambda, bad);
	} catch(std::runtime_error&) {
		b_thrown = true;
	}
	CHECK(b_thrown);
}

int main()
{
	{ // BA, cameras first: 3 cameras (6) with an odometry chain, 4 landmarks (3)
		std::vector<size_t> dims;
		dims.push_back(6); dims.push_back(6); dims.push_back(6);
		dims.push_back(3); dims.push_back(3); dims.push_back(3); dims.push_back(3);
		TBlockSet b;
		for(size_t c = 0; c < dims.size(); ++ c)
			b.insert(std::make_pair(c, c));
		b.insert(std::make_pair(size_t(0), size_t(1))); b.insert(std::make_pair(size_t(1), size_t(2)));
		b.insert(std::make_pair(size_t(0), size_t(3))); b.insert(std::make_pair(size_t(1), size_t(3)));
		b.insert(std::make_pair(size_t(1), size_t(4))); b.insert(std::make_pair(size_t(2), size_t(4)));
		b.insert(std::make_pair(size_t(0), size_t(5))); b.insert(std::make_pair(size_t(2), size_t(5)));
		b.insert(std::make_pair(size_t(2), size_t(6)));
		Check_System(dims, b, true, "cameras first");
	}
	{ // BA, cameras (6) and landmarks (3) interleaved: the class reorders, the library sees the cameras first
		std::vector<size_t> dims;
		dims.push_back(6); dims.push_back(3); dims.push_back(6); dims.push_back(3);
		dims.push_back(3); dims.push_back(6); dims.push_back(3);
		TBlockSet b;
		for(size_t c = 0; c < dims.size(); ++ c)
			b.insert(std::make_pair(c, c));
		b.insert(std::make_pair(size_t(0), size_t(1))); b.insert(std::make_pair(size_t(1), size_t(2)));  // landmark 1: cameras 0, 2
		b.insert(std::make_pair(size_t(2), size_t(3))); b.insert(std::make_pair(size_t(3), size_t(5)));  // landmark 3: cameras 2, 5
		b.insert(std::make_pair(size_t(0), size_t(4))); b.insert(std::make_pair(size_t(4), size_t(5)));  // landmark 4: cameras 0, 5
		b.insert(std::make_pair(size_t(5), size_t(6)));                                                  // landmark 6: camera 5
		b.insert(std::make_pair(size_t(0), size_t(2))); b.insert(std::make_pair(size_t(2), size_t(5)));  // camera chain
		Check_System(dims, b, true, "interleaved");
	}
	{ // no landmark part (every block column as wide): the class's sparse solver answers, the same way
		std::vector<size_t> dims(5, 6);
		TBlockSet b;
		for(size_t c = 0; c < dims.size(); ++ c) {
			b.insert(std::make_pair(c, c));
			if(c)
				b.insert(std::make_pair(c - 1, c));
		}
		b.insert(std::make_pair(size_t(0), size_t(3)));
		Check_System(dims, b, false, "no landmark part");
	}
	if(n_failures) {
		fprintf(stderr, "%d failures\n", n_failures);
		return 1;
	}
	printf("ok\n");
	return 0;
}
