// covariance_header_driver.cpp -- runs the covariance parts of include/slam/LinearSolver_HIP.h (Marginals with an
// EBlockMatrixPart, Marginal_Columns) on the CPU against stand-ins for the C ABI: the stand-ins answer every covariance
// request with a known symmetric matrix S(r, c), so the driver checks which blocks the header writes where, and with what.
// Built and run by tests/test_covariance_header.py against the reference's block matrix.  Prints "ok" and exits 0.
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

static double S(int64_t r, int64_t c) // the "covariance": symmetric, every entry distinct
{
	const int64_t a = std::min(r, c), b = std::max(r, c);
	return double(a) * 1009 + double(b) + 0.25;
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
				*out ++ = S(p->cumsum[c] + r, p->cumsum[c] + q);
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
					*out ++ = S(p->cumsum[R] + r, p->cumsum[c] + q);
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
				*out ++ = S(r, s);
	}
	return SLAMPP_HIP_OK;
}
} // extern "C"

// ---- the checks ----

static int n_failures = 0;
#define CHECK(c) do { if(!(c)) { fprintf(stderr, "failed at line %d: %s\n", __LINE__, #c); ++ n_failures; } } while(0)

// the blocks of r_m must be exactly r_expected (i, j) (upper triangle), each equal to S on its rows and columns
static void Check_Blocks(const CUberBlockMatrix &r_m, const CUberBlockMatrix &r_lambda, const std::set<std::pair<size_t, size_t> > &r_expected,
	const char *p_s_what)
{
	std::set<std::pair<size_t, size_t> > found;
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

int main()
{
	// lambda: 6 block columns of sizes 3, 2, 3, 3, 2, 3; a chain plus the chords (0, 3) and (2, 5)
	const size_t dims[] = {3, 2, 3, 3, 2, 3}, n = 6;
	std::set<std::pair<size_t, size_t> > lam_blocks;
	for(size_t c = 0; c < n; ++ c) {
		lam_blocks.insert(std::make_pair(c, c));
		if(c)
			lam_blocks.insert(std::make_pair(c - 1, c));
	}
	lam_blocks.insert(std::make_pair(size_t(0), size_t(3)));
	lam_blocks.insert(std::make_pair(size_t(2), size_t(5)));
	CUberBlockMatrix lambda;
	for(size_t c = 0; c < n; ++ c) {
		for(size_t r = 0; r <= c; ++ r) {
			if(!lam_blocks.count(std::make_pair(r, c)))
				continue;
			double *p = lambda.p_GetBlock_Log(r, c, dims[r], dims[c], true, false);
			CHECK(p != 0);
			for(size_t e = 0; p && e < dims[r] * dims[c]; ++ e)
				p[e] = (r == c && e % (dims[c] + 1) == 0)? 10.0 : 0.1;
		}
	}
	std::set<std::pair<size_t, size_t> > diag, last_block, last_col, full;
	for(size_t j = 0; j < n; ++ j) {
		diag.insert(std::make_pair(j, j));
		last_col.insert(std::make_pair(j, n - 1));
		for(size_t i = 0; i <= j; ++ i)
			full.insert(std::make_pair(i, j));
	}
	last_block.insert(std::make_pair(n - 1, n - 1));
	struct { int n_part; bool b_lambda; const std::set<std::pair<size_t, size_t> > *p_a, *p_b; const char *p_s_name; } cases[] = {
		{mpart_LastBlock, false, &last_block, 0, "mpart_LastBlock"},
		{mpart_LastColumn, false, &last_col, 0, "mpart_LastColumn"},
		{mpart_Diagonal, false, &diag, 0, "mpart_Diagonal"},
		{mpart_LastColumn | mpart_Diagonal, false, &last_col, &diag, "mpart_LastColumn | mpart_Diagonal"},
		{mpart_LastBlock | mpart_Diagonal, false, &last_block, &diag, "mpart_LastBlock | mpart_Diagonal"},
		{mpart_FullMatrix, false, &full, 0, "mpart_FullMatrix"},
		{mpart_LastBlock, true, &last_block, &lam_blocks, "mpart_LastBlock + lambda's structure"},
		{mpart_LastColumn, true, &last_col, &lam_blocks, "mpart_LastColumn + lambda's structure"},
		{mpart_Nothing, true, &lam_blocks, 0, "lambda's structure"}
	};
	CLinearSolver_HIP solver;
	for(size_t t = 0; t < sizeof(cases) / sizeof(cases[0]); ++ t) {
		std::set<std::pair<size_t, size_t> > expected(*cases[t].p_a);
		if(cases[t].p_b)
			expected.insert(cases[t].p_b->begin(), cases[t].p_b->end());
		CUberBlockMatrix marginals;
		bool b_ok = false;
		try {
			b_ok = solver.Marginals(marginals, lambda, EBlockMatrixPart(cases[t].n_part), cases[t].b_lambda);
		} catch(std::exception &r_exc) {
			fprintf(stderr, "%s: %s\n", cases[t].p_s_name, r_exc.what());
		}
		CHECK(b_ok);
		if(b_ok)
			Check_Blocks(marginals, lambda, expected, cases[t].p_s_name);
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
	// Marginal_Columns: n_scalars x k, the listed columns in order
	Eigen::MatrixXd X;
	std::vector<size_t> cols;
	cols.push_back(4);
	cols.push_back(0);
	CHECK(solver.Marginal_Columns(X, lambda, cols));
	CHECK(size_t(X.rows()) == lambda.n_Column_Num() && X.cols() == 5);
	for(int c = 0; c < X.cols(); ++ c) {
		const int64_t s = (c < 2)? int64_t(lambda.n_BlockColumn_Base(4)) + c : c - 2;
		for(int r = 0; r < X.rows(); ++ r)
			CHECK(X(r, c) == S(r, s));
	}
	if(n_failures) {
		fprintf(stderr, "%d failures\n", n_failures);
		return 1;
	}
	printf("ok\n");
	return 0;
}
