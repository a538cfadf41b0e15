// capi_standins.h -- stand-ins for the C ABI (include/slampp_hip.h) that the header binding include/slam/LinearSolver_HIP.h
// calls, for drivers that run the binding on the CPU: every covariance request is answered with a known symmetric matrix
// S(r, c) of lambda's scalars, seen through the ordering the binding hands the library, so a driver can check which blocks
// the binding writes where, and with what.  Also what such drivers share: the failure count, lambdas of a given pattern
// and the check of a block matrix against S.  Include it once, in the driver's only translation unit.
#pragma once
#include "slam/LinearSolver_HIP.h"
#include <cmath>
#include <set>

static int n_failures = 0;
#define CHECK(c) do { if(!(c)) { fprintf(stderr, "failed at line %d: %s\n", __LINE__, #c); ++ n_failures; } } while(0)

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

// the library sees lambda in the order the binding hands over: its scalar s is lambda's scalar g_lambda_scalar[s] (empty: the same)
static std::vector<int64_t> g_lambda_scalar;
static int g_n_schur_calls = 0; // calls of the Schur covariance stand-ins
static int g_n_flipped = 0; // pairs r < c of lambda that reached the Schur pair stand-in as r' > c'

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
int slampp_hip_marginal_blocks(slampp_hip_solver *p, const double *, int64_t n_pairs, const int64_t *brows, const int64_t *bcols, double *out)
{
	const int64_t n = int64_t(p->cumsum.size()) - 1;
	if(n_pairs <= 0 || !brows || !bcols || !out)
		return SLAMPP_HIP_ERR_INVALID;
	for(int64_t k = 0; k < n_pairs; ++ k) {
		const int64_t R = brows[k], C = bcols[k];
		if(R < 0 || R >= n || C < 0 || C >= n)
			return SLAMPP_HIP_ERR_INVALID;
		for(int64_t q = p->cumsum[size_t(C)]; q < p->cumsum[size_t(C) + 1]; ++ q)
			for(int64_t r = p->cumsum[size_t(R)]; r < p->cumsum[size_t(R) + 1]; ++ r)
				*out ++ = S_lib(r, q);
	}
	return SLAMPP_HIP_OK;
}
int slampp_hip_schur_marginals_pattern(slampp_hip_solver *p, const double *, double *out)
{
	++ g_n_schur_calls;
	return slampp_hip_marginals_pattern(p, 0, out);
}
int slampp_hip_schur_marginal_columns(slampp_hip_solver *p, const double *, int n_cols, const int64_t *bcols, double *out)
{
	++ g_n_schur_calls;
	return slampp_hip_marginal_columns(p, 0, n_cols, bcols, out);
}
int slampp_hip_schur_marginal_blocks(slampp_hip_solver *p, const double *, int64_t n_pairs, const int64_t *brows, const int64_t *bcols,
	double *out)
{
	++ g_n_schur_calls;
	for(int64_t k = 0; brows && bcols && k < n_pairs; ++ k) {
		if(!g_lambda_scalar.empty() && brows[k] >= 0 && bcols[k] >= 0 && size_t(brows[k]) + 1 < p->cumsum.size() &&
		   size_t(bcols[k]) + 1 < p->cumsum.size() && (brows[k] > bcols[k]) !=
		   (g_lambda_scalar[size_t(p->cumsum[size_t(brows[k])])] > g_lambda_scalar[size_t(p->cumsum[size_t(bcols[k])])]))
			++ g_n_flipped;
	}
	return slampp_hip_marginal_blocks(p, 0, n_pairs, brows, bcols, out);
}
} // extern "C"

typedef std::set<std::pair<size_t, size_t> > TBlockSet;

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

// tells the stand-ins the order the library sees r_lambda in: b_guided: the guided ordering of the Schur class (the widest
// block columns first, then the others, both in stable order); otherwise lambda's own
static void Set_Library_Order(const CUberBlockMatrix &r_lambda, const std::vector<size_t> &r_dims, bool b_guided)
{
	g_lambda_scalar.clear();
	const size_t n_wide = *std::max_element(r_dims.begin(), r_dims.end());
	for(int n_pass = 0; b_guided && n_pass < 2; ++ n_pass) {
		for(size_t i = 0; i < r_dims.size(); ++ i) {
			for(size_t d = 0; (r_dims[i] == n_wide) == !n_pass && d < r_dims[i]; ++ d)
				g_lambda_scalar.push_back(int64_t(r_lambda.n_BlockColumn_Base(i) + d));
		}
	}
}

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
