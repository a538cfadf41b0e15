// capi_resolve.hip -- the entry points of the C ABI (include/slampp_hip.h) that work with a factor or beside one: the factor
// handed out (slampp_hip_factorize, slampp_hip_factor_structure), further right-hand sides with the kept factor
// (slampp_hip_solve_again; several at once: slampp_hip_solve_columns; one substitution at a time: slampp_hip_solve_half_columns,
// with the Gram product slampp_hip_gram_device_async), y = alpha Lambda x + beta y and its adjoint in the values (the outer product on Lambda's pattern),
// dot products and iterative refinement
#include "capi_util.h"
#include "covariance.h"
#include "multiply.h"
#include "gram.h"
#include "pattern_outer.h"

#include <algorithm>

using namespace slampp;

extern "C" {

// The factor's block structure in the CALLER's block columns (what slampp_hip_factorize fills).  Without wide columns that is
// the plan's own; where block columns wider than 8 were cut into pieces (Refine_Structure) the pieces are put together
// again: block (I, J) of the caller's columns exists where any of its pieces does.  Needs the pieces of a column next to
// each other and in order, which the caller's own order (option natural_order; what Factorize_PosDef_Blocky asks for:
// the matrix comes pre-ordered, LinearSolver_CholMod.cpp:362-544) guarantees.
namespace {

struct TCoarseFactor {
	std::vector<int32_t> perm, dim, lrow;
	std::vector<int64_t> lptr, loff; // loff[l_blocks] = number of values
	std::vector<int32_t> piece_col, piece_off; // refined column -> caller's column, scalar offset inside it
};

bool coarse_factor_structure(const slampp_hip_solver &s, TCoarseFactor &r_out, std::string &r_s_why)
{
	const Plan &P = s.plan;
	const int64_t n = int64_t(s.cumsum.size()) - 1, n_refined = int64_t(s.refined_cumsum.size()) - 1;
	r_out.piece_col.assign(size_t(n_refined), 0);
	r_out.piece_off.assign(size_t(n_refined), 0);
	{
		int64_t c = 0;
		for(int64_t p = 0; p < n_refined; ++ p) {
			while(s.refined_cumsum[p] >= s.cumsum[c + 1])
				++ c;
			r_out.piece_col[p] = int32_t(c);
			r_out.piece_off[p] = int32_t(s.refined_cumsum[p] - s.cumsum[c]);
		}
	}
	for(int64_t p = 0; p < n_refined; ++ p) {
		if(P.perm[p] != p) {
			r_s_why = "factorize: block columns wider than 8 are factored in pieces: the factor has the caller's block layout only in the caller's own order (option natural_order = 1)";
			return false;
		}
	}
	r_out.perm.resize(size_t(n));
	r_out.dim.resize(size_t(n));
	for(int64_t c = 0; c < n; ++ c) {
		r_out.perm[c] = int32_t(c);
		r_out.dim[c] = int32_t(s.cumsum[c + 1] - s.cumsum[c]);
	}
	r_out.lptr.assign(1, 0);
	r_out.lrow.clear();
	r_out.loff.clear();
	std::vector<int32_t> rows;
	int64_t n_off = 0, p = 0;
	for(int64_t c = 0; c < n; ++ c) {
		rows.clear();
		for(; p < n_refined && r_out.piece_col[p] == c; ++ p) {
			for(int64_t k = P.lptr[p]; k < P.lptr[p + 1]; ++ k)
				rows.push_back(r_out.piece_col[P.lrow[k]]);
		}
		std::sort(rows.begin(), rows.end());
		rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
		for(size_t i = 0; i < rows.size(); ++ i) { // (ascending: the diagonal block first)
			r_out.lrow.push_back(rows[i]);
			r_out.loff.push_back(n_off);
			n_off += int64_t(r_out.dim[rows[i]]) * r_out.dim[c];
		}
		r_out.lptr.push_back(int64_t(r_out.lrow.size()));
	}
	r_out.loff.push_back(n_off);
	return true;
}

} // anonymous namespace

int slampp_hip_factor_structure(const slampp_hip_solver *p_solver, int64_t *p_n_bcols, int64_t *p_l_blocks, int64_t *p_l_values,
	int32_t *p_perm, int32_t *p_dim, int64_t *p_lptr, int32_t *p_lrow, int64_t *p_loff)
{
	if(!p_solver || !p_solver->b_analyzed || p_solver->n_mode != SLAMPP_HIP_MODE_SPARSE)
		return SLAMPP_HIP_ERR_INVALID;
	const slampp_hip_solver &s = *p_solver;
	const Plan &P = s.plan;
	try {
		if(!s.b_refined) {
			if(p_n_bcols) *p_n_bcols = P.n;
			if(p_l_blocks) *p_l_blocks = int64_t(P.lrow.size());
			if(p_l_values) *p_l_values = P.loff[P.lrow.size()];
			if(p_perm) std::copy(P.perm.begin(), P.perm.end(), p_perm);
			if(p_dim) std::copy(P.dim.begin(), P.dim.end(), p_dim);
			if(p_lptr) std::copy(P.lptr.begin(), P.lptr.end(), p_lptr);
			if(p_lrow) std::copy(P.lrow.begin(), P.lrow.end(), p_lrow);
			if(p_loff) std::copy(P.loff.begin(), P.loff.begin() + P.lrow.size(), p_loff);
			return SLAMPP_HIP_OK;
		}
		TCoarseFactor t;
		std::string s_why;
		if(!coarse_factor_structure(s, t, s_why)) {
			const_cast<slampp_hip_solver*>(p_solver)->s_error = s_why;
			return SLAMPP_HIP_ERR_UNSUPPORTED;
		}
		if(p_n_bcols) *p_n_bcols = int64_t(t.dim.size());
		if(p_l_blocks) *p_l_blocks = int64_t(t.lrow.size());
		if(p_l_values) *p_l_values = t.loff.back();
		if(p_perm) std::copy(t.perm.begin(), t.perm.end(), p_perm);
		if(p_dim) std::copy(t.dim.begin(), t.dim.end(), p_dim);
		if(p_lptr) std::copy(t.lptr.begin(), t.lptr.end(), p_lptr);
		if(p_lrow) std::copy(t.lrow.begin(), t.lrow.end(), p_lrow);
		if(p_loff) std::copy(t.loff.begin(), t.loff.end() - 1, p_loff);
		return SLAMPP_HIP_OK;
	} catch(std::bad_alloc&) {
		return SLAMPP_HIP_ERR_ALLOC;
	}
}

int slampp_hip_factorize(slampp_hip_solver *p_solver, const double *p_values, double *p_factor_out)
{
	TCoarseFactor t; // (block columns wider than 8 only: how their pieces go together, and the pieces as the device holds them)
	std::vector<double> pieces;
	const int n_result = host_round_trip(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		if(!s.b_analyzed)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "factorize: analyze was not called");
		if(s.n_mode != SLAMPP_HIP_MODE_SPARSE)
			return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, "factorize: the sparse mode only");
		if(!p_values || !p_factor_out)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "factorize: null pointer");
		if(s.b_refined) {
			for(size_t p = 0; p < s.plan.perm.size(); ++ p) {
				if(s.plan.perm[p] != int32_t(p))
					return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, "factorize: block columns wider than 8 are factored in pieces: the factor has the caller's block layout only in the caller's own order (option natural_order = 1)");
			}
		}
		s.d_A.Alloc(size_t(s.n_values));
		s.d_rhs.Alloc(size_t(s.n_scalars));
		Upload_Values_And_Join(s, p_values);
		SLAMPP_HIP_CHECK(hipMemsetAsync(s.d_rhs.p(), 0, size_t(s.n_scalars) * sizeof(double), s.stream)); // the fused forward substitution runs on zeros
		s.Enqueue_Sparse(s.d_A.p(), s.d_rhs.p(), true, true); // (a dense top factors its columns on the matrix cores and hands them back into the block layout)
		s.Factor_Installed(s.n_dense_dim == 0); // (with a dense top the substitutions' vectors were not brought along: no solve_again from this)
		return SLAMPP_HIP_OK;
	}, [](slampp_hip_solver&) { return SLAMPP_HIP_OK; } /* (enqueued above: this entry point has no device twin) */, true, [&](slampp_hip_solver &s) {
		const size_t n_l_values = size_t(s.plan.loff[s.plan.lrow.size()]);
		if(!s.b_refined) {
			SLAMPP_HIP_CHECK(hipMemcpyAsync(p_factor_out, s.d_L.p(), n_l_values * sizeof(double), hipMemcpyDeviceToHost, s.stream));
			return;
		}
		std::string s_why;
		if(!coarse_factor_structure(s, t, s_why))
			throw std::domain_error(s_why); // (SLAMPP_HIP_ERR_UNSUPPORTED, with this message)
		pieces.resize(n_l_values);
		SLAMPP_HIP_CHECK(hipMemcpyAsync(pieces.data(), s.d_L.p(), n_l_values * sizeof(double), hipMemcpyDeviceToHost, s.stream));
	});
	if(n_result != SLAMPP_HIP_OK || !p_solver->b_refined)
		return n_result;
	// the pieces of the wide columns put together again: piece block (pi, pj) is a sub-block of the caller's block (I, J)
	const Plan &P = p_solver->plan;
	std::fill(p_factor_out, p_factor_out + t.loff.back(), 0.0);
	for(int64_t pj = 0; pj < int64_t(P.n); ++ pj) {
		const int32_t J = t.piece_col[pj];
		const int n_col0 = t.piece_off[pj], w = P.dim[pj];
		for(int64_t k = P.lptr[pj]; k < P.lptr[pj + 1]; ++ k) {
			const int32_t pi = P.lrow[k], I = t.piece_col[pi];
			const int n_row0 = t.piece_off[pi], h = P.dim[pi], H = t.dim[I];
			const int32_t *p_first = &t.lrow[size_t(t.lptr[J])], *p_last = &t.lrow[size_t(t.lptr[J + 1])];
			const int64_t n_blk = t.lptr[J] + (std::lower_bound(p_first, p_last, I) - p_first);
			double *p_dst = p_factor_out + t.loff[size_t(n_blk)];
			const double *p_src = &pieces[size_t(P.loff[k])];
			for(int b = 0; b < w; ++ b) {
				for(int a = 0; a < h; ++ a)
					p_dst[(n_row0 + a) + size_t(n_col0 + b) * H] = p_src[a + size_t(b) * h];
			}
		}
	}
	return SLAMPP_HIP_OK;
}

namespace {

// Schur mode: which kept state another right-hand side can be solved from (inside guarded()).  0 = none; 1 = what a solve
// with "schur_keep" / "schur_incremental" left; 2 = what a Schur covariance call left.  Both are generations of
// n_factor_gen: whatever installs or drops a factor since (a solve, a batch, marginals, a factorization that turns out not
// positive definite at slampp_hip_sync, set_structure, analyze) counts it up and thereby ends them.
int schur_resolve_source(const slampp_hip_solver &s)
{
	if(!s.p_schur || !s.n_factor_gen)
		return 0;
	if(s.n_schur_keep_gen == s.n_factor_gen)
		return 1;
	if(s.n_schur_cov_gen == s.n_factor_gen)
		return 2;
	return 0;
}

// the checks of slampp_hip_solve_again_device_async / slampp_hip_refine (inside guarded()): SLAMPP_HIP_OK, and how to solve
int resolve_checks(slampp_hip_solver *p_solver, const char *p_s_name, int *p_n_schur_source)
{
	slampp_hip_solver &s = *p_solver;
	const std::string s_name(p_s_name);
	*p_n_schur_source = 0;
	if(s.b_group_active || (s.n_mode == SLAMPP_HIP_MODE_SCHUR && s.p_allreduce))
		return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, (s_name + ": not for a handle that solves with landmark shards or over several devices").c_str());
	if(!s.b_analyzed)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, (s_name + ": no valid factorization (analyze was not called)").c_str());
	if(s.n_mode == SLAMPP_HIP_MODE_SPARSE) {
		if(!s.b_factored)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, (s_name + ": no valid factorization").c_str());
		return SLAMPP_HIP_OK;
	}
	if(!(*p_n_schur_source = schur_resolve_source(s)))
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, (s_name + ": no kept factor of the reduced camera system: set the option schur_keep (or "
			"schur_incremental) before analyze and solve, or call a Schur covariance entry point; anything that factors or fails "
			"to since ends its validity").c_str());
	return SLAMPP_HIP_OK;
}

// the substitutions themselves, enqueue-only
void resolve_enqueue(slampp_hip_solver &s, double *p_rhs_dev, int n_schur_source)
{
	if(s.n_mode == SLAMPP_HIP_MODE_SPARSE)
		s.Enqueue_Sparse(0, p_rhs_dev, false);
	else
		schur_resolve_enqueue(s, p_rhs_dev, n_schur_source == 2);
}

} // anonymous namespace

int slampp_hip_solve_again_device_async(slampp_hip_solver *p_solver, double *p_rhs_inout_dev)
{
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		int n_source = 0;
		const int n_check = resolve_checks(p_solver, "solve_again", &n_source);
		if(n_check != SLAMPP_HIP_OK)
			return n_check;
		if(!p_rhs_inout_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "solve_again: null pointer");
		resolve_enqueue(s, p_rhs_inout_dev, n_source);
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_solve_again(slampp_hip_solver *p_solver, double *p_rhs_inout)
{
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		int n_source = 0;
		if(s.n_mode != SLAMPP_HIP_MODE_SPARSE && s.b_analyzed && !s.b_group_active && (n_source = schur_resolve_source(s))) {
			// Schur mode with W, C^-1 and the reduced system's factor kept: the same route as the device entry point
			const int n_check = resolve_checks(p_solver, "solve_again", &n_source);
			if(n_check != SLAMPP_HIP_OK)
				return n_check;
		} else {
			if(!s.b_factored)
				return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "solve_again: no valid factorization");
			if(s.n_mode != SLAMPP_HIP_MODE_SPARSE)
				return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, "solve_again: only the sparse path keeps its factor");
		}
		if(!p_rhs_inout)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "solve_again: null pointer");
		s.d_rhs.Alloc(size_t(s.n_scalars));
		SLAMPP_HIP_CHECK(hipMemcpyAsync(s.d_rhs.p(), p_rhs_inout, size_t(s.n_scalars) * sizeof(double), hipMemcpyHostToDevice, s.stream));
		resolve_enqueue(s, s.d_rhs.p(), n_source);
		SLAMPP_HIP_CHECK(hipMemcpyAsync(p_rhs_inout, s.d_rhs.p(), size_t(s.n_scalars) * sizeof(double), hipMemcpyDeviceToHost, s.stream));
		SLAMPP_HIP_CHECK(hipStreamSynchronize(s.stream));
		return SLAMPP_HIP_OK;
	});
}

// ---- several right-hand sides with the kept factor in one call (covariance.hip: solve_columns_enqueue) ----

namespace {

// the checks of both solve_columns entry points (inside guarded())
int solve_columns_checks(slampp_hip_solver *p_solver, const double *p_rhs, int64_t n_ld, int n_columns, int *p_n_schur_source)
{
	const int n_check = resolve_checks(p_solver, "solve_columns", p_n_schur_source);
	if(n_check != SLAMPP_HIP_OK)
		return n_check;
	if(!p_rhs)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "solve_columns: null pointer");
	if(n_columns < 1 || n_columns > SLAMPP_HIP_SOLVE_MAX_COLUMNS)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "solve_columns: between 1 and SLAMPP_HIP_SOLVE_MAX_COLUMNS columns");
	if(n_columns > 1 && n_ld < p_solver->n_scalars)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "solve_columns: the columns overlap (leading dimension below n_scalars)");
	return SLAMPP_HIP_OK;
}

} // anonymous namespace

int slampp_hip_solve_columns_device_async(slampp_hip_solver *p_solver, double *p_rhs_inout_dev, int64_t n_ld, int n_columns)
{
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		int n_source = 0;
		const int n_check = solve_columns_checks(p_solver, p_rhs_inout_dev, n_ld, n_columns, &n_source);
		if(n_check != SLAMPP_HIP_OK)
			return n_check;
		if(s.n_mode == SLAMPP_HIP_MODE_SPARSE && solve_columns_applies(s))
			solve_columns_enqueue(s, p_rhs_inout_dev, n_ld, n_columns);
		else { // Schur mode, block columns wider than 8: the single-vector route, column by column (slampp_hip_solve_again's bits)
			for(int c = 0; c < n_columns; ++ c)
				resolve_enqueue(s, p_rhs_inout_dev + int64_t(c) * n_ld, n_source);
		}
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_solve_columns(slampp_hip_solver *p_solver, double *p_rhs_inout, int64_t n_ld, int n_columns)
{
	// groups of at most COV_K_PASS columns, each through the device array of the covariance columns (packed there) and back
	// behind its pass: the device holds n_scalars x COV_K_PASS of them at a time, whatever n_columns is
	int n_group0 = 0, n_group = n_columns;
	do {
		const int n_result = host_round_trip(p_solver, [&]() -> int {
			slampp_hip_solver &s = *p_solver;
			int n_source = 0;
			const int n_check = solve_columns_checks(p_solver, p_rhs_inout, n_ld, n_columns, &n_source);
			if(n_check != SLAMPP_HIP_OK)
				return n_check;
			n_group = std::min(n_columns - n_group0, int(COV_K_PASS));
			s.d_cov.Alloc(size_t(s.n_scalars) * n_group);
			SLAMPP_HIP_CHECK(hipMemcpy2DAsync(s.d_cov.p(), size_t(s.n_scalars) * sizeof(double), p_rhs_inout + int64_t(n_group0) * n_ld,
				size_t(std::max(n_ld, s.n_scalars)) * sizeof(double) /* (one column: n_ld is of no meaning) */, size_t(s.n_scalars) * sizeof(double), size_t(n_group), hipMemcpyHostToDevice, s.stream));
			return SLAMPP_HIP_OK;
		}, [&](slampp_hip_solver &s) {
			return slampp_hip_solve_columns_device_async(p_solver, s.d_cov.p(), s.n_scalars, n_group);
		}, false, [&](slampp_hip_solver &s) {
			SLAMPP_HIP_CHECK(hipMemcpy2DAsync(p_rhs_inout + int64_t(n_group0) * n_ld, size_t(std::max(n_ld, s.n_scalars)) * sizeof(double), s.d_cov.p(),
				size_t(s.n_scalars) * sizeof(double), size_t(s.n_scalars) * sizeof(double), size_t(n_group), hipMemcpyDeviceToHost, s.stream));
		});
		if(n_result != SLAMPP_HIP_OK)
			return n_result;
		n_group0 += n_group;
	} while(n_group0 < n_columns);
	return SLAMPP_HIP_OK;
}

// ---- one substitution at a time on the kept factor (covariance.hip: solve_half_columns_enqueue) ----

namespace {

// the checks of both solve_half_columns entry points (inside guarded())
int solve_half_columns_checks(slampp_hip_solver *p_solver, int n_half, const double *p_inout, int64_t n_ld, int n_columns)
{
	int n_source = 0;
	const int n_check = resolve_checks(p_solver, "solve_half_columns", &n_source);
	if(n_check != SLAMPP_HIP_OK)
		return n_check;
	if(n_half != SLAMPP_HIP_HALF_FORWARD && n_half != SLAMPP_HIP_HALF_BACKWARD)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "solve_half_columns: n_half is SLAMPP_HIP_HALF_FORWARD or SLAMPP_HIP_HALF_BACKWARD");
	if(!p_inout)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "solve_half_columns: null pointer");
	if(n_columns < 1 || n_columns > SLAMPP_HIP_SOLVE_MAX_COLUMNS)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "solve_half_columns: between 1 and SLAMPP_HIP_SOLVE_MAX_COLUMNS columns");
	if(n_columns > 1 && n_ld < p_solver->n_scalars)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "solve_half_columns: the columns overlap (leading dimension below n_scalars)");
	if(p_solver->n_mode != SLAMPP_HIP_MODE_SPARSE)
		return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, "solve_half_columns: not in Schur mode: the factor there is the block factor "
			"[L_S, U L_C^-T; 0, L_C], whose halves need the Cholesky factor L_C of every landmark block (kept is C^-1)");
	if(!solve_columns_applies(*p_solver))
		return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, "solve_half_columns: block columns wider than 8 are factored in pieces: "
			"no k-column kernels run on them, and the factor's row order is not the caller's blocks'");
	return SLAMPP_HIP_OK;
}

} // anonymous namespace

int slampp_hip_solve_half_columns_device_async(slampp_hip_solver *p_solver, int n_half, double *p_inout_dev, int64_t n_ld, int n_columns)
{
	return guarded(p_solver, [&]() -> int {
		const int n_check = solve_half_columns_checks(p_solver, n_half, p_inout_dev, n_ld, n_columns);
		if(n_check != SLAMPP_HIP_OK)
			return n_check;
		solve_half_columns_enqueue(*p_solver, n_half == SLAMPP_HIP_HALF_BACKWARD, p_inout_dev, n_ld, n_columns);
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_solve_half_columns(slampp_hip_solver *p_solver, int n_half, double *p_inout, int64_t n_ld, int n_columns)
{
	// groups of at most COV_K_PASS columns through the device array of the covariance columns, as slampp_hip_solve_columns
	int n_group0 = 0, n_group = n_columns;
	do {
		const int n_result = host_round_trip(p_solver, [&]() -> int {
			slampp_hip_solver &s = *p_solver;
			const int n_check = solve_half_columns_checks(p_solver, n_half, p_inout, n_ld, n_columns);
			if(n_check != SLAMPP_HIP_OK)
				return n_check;
			n_group = std::min(n_columns - n_group0, int(COV_K_PASS));
			s.d_cov.Alloc(size_t(s.n_scalars) * n_group);
			SLAMPP_HIP_CHECK(hipMemcpy2DAsync(s.d_cov.p(), size_t(s.n_scalars) * sizeof(double), p_inout + int64_t(n_group0) * n_ld,
				size_t(std::max(n_ld, s.n_scalars)) * sizeof(double) /* (one column: n_ld is of no meaning) */, size_t(s.n_scalars) * sizeof(double), size_t(n_group), hipMemcpyHostToDevice, s.stream));
			return SLAMPP_HIP_OK;
		}, [&](slampp_hip_solver &s) {
			return slampp_hip_solve_half_columns_device_async(p_solver, n_half, s.d_cov.p(), s.n_scalars, n_group);
		}, false, [&](slampp_hip_solver &s) {
			SLAMPP_HIP_CHECK(hipMemcpy2DAsync(p_inout + int64_t(n_group0) * n_ld, size_t(std::max(n_ld, s.n_scalars)) * sizeof(double), s.d_cov.p(),
				size_t(s.n_scalars) * sizeof(double), size_t(s.n_scalars) * sizeof(double), size_t(n_group), hipMemcpyDeviceToHost, s.stream));
		});
		if(n_result != SLAMPP_HIP_OK)
			return n_result;
		n_group0 += n_group;
	} while(n_group0 < n_columns);
	return SLAMPP_HIP_OK;
}

// ---- y = alpha Lambda x + beta y, dot products, iterative refinement (multiply.hip) ----

namespace {

int multiply_checks(slampp_hip_solver *p_solver, const char *p_s_name)
{
	slampp_hip_solver &s = *p_solver;
	const std::string s_name(p_s_name);
	if(!s.b_has_structure)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, (s_name + ": set_structure was not called").c_str());
	if(s.b_group_active)
		return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, (s_name + ": this handle solves with landmark shards on several devices").c_str());
	return SLAMPP_HIP_OK;
}

} // anonymous namespace

int slampp_hip_multiply_device_async(slampp_hip_solver *p_solver, const double *p_values_dev, const double *p_x_dev,
	double *p_y_dev, double f_alpha, double f_beta)
{
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		const int n_check = multiply_checks(p_solver, "multiply");
		if(n_check != SLAMPP_HIP_OK)
			return n_check;
		if(!p_values_dev || !p_x_dev || !p_y_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "multiply: null pointer");
		if(p_x_dev == p_y_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "multiply: x and y must be different vectors (every row of y reads all of x)");
		s.Require_Multiply();
		multiply_enqueue(*s.p_mul, p_values_dev, p_x_dev, p_y_dev, f_alpha, f_beta, s.stream);
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_multiply(slampp_hip_solver *p_solver, const double *p_values, const double *p_x, double *p_y, double f_alpha,
	double f_beta)
{
	return host_round_trip(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		const int n_check = multiply_checks(p_solver, "multiply");
		if(n_check != SLAMPP_HIP_OK)
			return n_check;
		if(!p_values || !p_x || !p_y)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "multiply: null pointer");
		if(p_x == p_y)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "multiply: x and y must be different vectors (every row of y reads all of x)");
		const size_t n_bytes = size_t(s.n_scalars) * sizeof(double);
		s.d_A.Alloc(size_t(s.n_values));
		s.d_mul_x.Alloc(size_t(s.n_scalars));
		s.d_mul_y.Alloc(size_t(s.n_scalars));
		Upload_Values_And_Join(s, p_values);
		SLAMPP_HIP_CHECK(hipMemcpyAsync(s.d_mul_x.p(), p_x, n_bytes, hipMemcpyHostToDevice, s.stream));
		if(f_beta != 0)
			SLAMPP_HIP_CHECK(hipMemcpyAsync(s.d_mul_y.p(), p_y, n_bytes, hipMemcpyHostToDevice, s.stream));
		return SLAMPP_HIP_OK;
	}, [&](slampp_hip_solver &s) {
		return slampp_hip_multiply_device_async(p_solver, s.d_A.p(), s.d_mul_x.p(), s.d_mul_y.p(), f_alpha, f_beta);
	}, false, [&](slampp_hip_solver &s) {
		SLAMPP_HIP_CHECK(hipMemcpyAsync(p_y, s.d_mul_y.p(), size_t(s.n_scalars) * sizeof(double), hipMemcpyDeviceToHost, s.stream));
	});
}

// ---- out = alpha P(a, b) + beta out on Lambda's pattern (pattern_outer.hip) ----

namespace {

// do [p_a, p_a + n_a) and [p_b, p_b + n_b) share an element?
bool ranges_overlap(const double *p_a, int64_t n_a, const double *p_b, int64_t n_b)
{
	const uintptr_t a0 = reinterpret_cast<uintptr_t>(p_a), b0 = reinterpret_cast<uintptr_t>(p_b);
	return a0 < b0 + uintptr_t(n_b) * sizeof(double) && b0 < a0 + uintptr_t(n_a) * sizeof(double);
}

} // anonymous namespace

int slampp_hip_pattern_outer_batch_device_async(slampp_hip_solver *p_solver, int n_batch, const double *p_a_dev, int64_t n_a_stride,
	const double *p_b_dev, int64_t n_b_stride, double *p_out_values_dev, int64_t n_out_stride, double f_alpha, double f_beta)
{
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		const int n_check = multiply_checks(p_solver, "pattern_outer");
		if(n_check != SLAMPP_HIP_OK)
			return n_check;
		if(!p_a_dev || !p_b_dev || !p_out_values_dev || n_batch < 1 || n_batch > SLAMPP_HIP_MAX_BATCH)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "pattern_outer: null pointer, or a batch of fewer than 1 / more than SLAMPP_HIP_MAX_BATCH members");
		if(n_batch == 1)
			n_a_stride = n_b_stride = n_out_stride = 0; // (of no meaning)
		else if(n_a_stride < s.n_scalars || n_b_stride < s.n_scalars || n_out_stride < s.n_values)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "pattern_outer: the members' vectors / values overlap (stride below their length)");
		const int64_t n_out_span = int64_t(n_batch - 1) * n_out_stride + s.n_values;
		if(ranges_overlap(p_a_dev, int64_t(n_batch - 1) * n_a_stride + s.n_scalars, p_out_values_dev, n_out_span) ||
		   ranges_overlap(p_b_dev, int64_t(n_batch - 1) * n_b_stride + s.n_scalars, p_out_values_dev, n_out_span))
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "pattern_outer: out overlaps a or b");
		s.Require_Pattern_Outer();
		pattern_outer_enqueue(*s.p_outer, n_batch, p_a_dev, n_a_stride, p_b_dev, n_b_stride, p_out_values_dev, n_out_stride, f_alpha,
			f_beta, s.stream);
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_pattern_outer_sum_device_async(slampp_hip_solver *p_solver, int n_terms, const double *p_a_dev, int64_t n_a_stride,
	const double *p_b_dev, int64_t n_b_stride, double *p_out_values_dev, double f_alpha, double f_beta)
{
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		const int n_check = multiply_checks(p_solver, "pattern_outer_sum");
		if(n_check != SLAMPP_HIP_OK)
			return n_check;
		if(!p_a_dev || !p_b_dev || !p_out_values_dev || n_terms < 1 || n_terms > SLAMPP_HIP_SOLVE_MAX_COLUMNS)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "pattern_outer_sum: null pointer, or fewer than 1 / more than SLAMPP_HIP_SOLVE_MAX_COLUMNS terms");
		if(n_terms == 1)
			n_a_stride = n_b_stride = 0; // (of no meaning)
		else if(n_a_stride < s.n_scalars || n_b_stride < s.n_scalars)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "pattern_outer_sum: the terms' vectors overlap (stride below their length)");
		if(ranges_overlap(p_a_dev, int64_t(n_terms - 1) * n_a_stride + s.n_scalars, p_out_values_dev, s.n_values) ||
		   ranges_overlap(p_b_dev, int64_t(n_terms - 1) * n_b_stride + s.n_scalars, p_out_values_dev, s.n_values))
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "pattern_outer_sum: out overlaps a or b");
		s.Require_Pattern_Outer();
		pattern_outer_sum_enqueue(*s.p_outer, n_terms, p_a_dev, n_a_stride, p_b_dev, n_b_stride, p_out_values_dev, f_alpha, f_beta, s.stream);
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_pattern_outer_device_async(slampp_hip_solver *p_solver, const double *p_a_dev, const double *p_b_dev,
	double *p_out_values_dev, double f_alpha, double f_beta)
{
	return slampp_hip_pattern_outer_batch_device_async(p_solver, 1, p_a_dev, 0, p_b_dev, 0, p_out_values_dev, 0, f_alpha, f_beta);
}

int slampp_hip_pattern_outer(slampp_hip_solver *p_solver, const double *p_a, const double *p_b, double *p_out_values, double f_alpha,
	double f_beta)
{
	return host_round_trip(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		const int n_check = multiply_checks(p_solver, "pattern_outer");
		if(n_check != SLAMPP_HIP_OK)
			return n_check;
		if(!p_a || !p_b || !p_out_values)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "pattern_outer: null pointer");
		if(ranges_overlap(p_a, s.n_scalars, p_out_values, s.n_values) || ranges_overlap(p_b, s.n_scalars, p_out_values, s.n_values))
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "pattern_outer: out overlaps a or b");
		const size_t n_bytes = size_t(s.n_scalars) * sizeof(double);
		s.d_mul_x.Alloc(size_t(s.n_scalars));
		s.d_mul_y.Alloc(size_t(s.n_scalars));
		s.d_outer_out.Alloc(size_t(s.n_values));
		SLAMPP_HIP_CHECK(hipMemcpyAsync(s.d_mul_x.p(), p_a, n_bytes, hipMemcpyHostToDevice, s.stream));
		SLAMPP_HIP_CHECK(hipMemcpyAsync(s.d_mul_y.p(), p_b, n_bytes, hipMemcpyHostToDevice, s.stream));
		if(f_beta != 0)
			SLAMPP_HIP_CHECK(hipMemcpyAsync(s.d_outer_out.p(), p_out_values, size_t(s.n_values) * sizeof(double), hipMemcpyHostToDevice, s.stream));
		return SLAMPP_HIP_OK;
	}, [&](slampp_hip_solver &s) {
		return slampp_hip_pattern_outer_device_async(p_solver, s.d_mul_x.p(), s.d_mul_y.p(), s.d_outer_out.p(), f_alpha, f_beta);
	}, false, [&](slampp_hip_solver &s) {
		SLAMPP_HIP_CHECK(hipMemcpyAsync(p_out_values, s.d_outer_out.p(), size_t(s.n_values) * sizeof(double), hipMemcpyDeviceToHost, s.stream));
	});
}

int slampp_hip_dot_device_async(slampp_hip_solver *p_solver, const double *p_a_dev, const double *p_b_dev, int64_t n,
	double *p_out_dev)
{
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		if(!p_a_dev || !p_b_dev || !p_out_dev || n < 0)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "dot: null pointer or negative length");
		if(s.b_group_active)
			return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, "dot: this handle solves with landmark shards on several devices");
		s.d_reduce.Alloc(reduce_MAX_PARTIALS);
		dot_enqueue(p_a_dev, p_b_dev, n, s.d_reduce.p(), p_out_dev, s.stream);
		return SLAMPP_HIP_OK;
	});
}

static_assert(SLAMPP_HIP_GRAM_MAX_COLUMNS == gram_MAX_COLUMNS && SLAMPP_HIP_GRAM_CHUNK_ROWS == gram_CHUNK_ROWS, "include/slampp_hip.h and gram.h disagree");

int slampp_hip_gram_device_async(slampp_hip_solver *p_solver, const double *p_a_dev, int64_t n_lda, int n_ka, const double *p_b_dev,
	int64_t n_ldb, int n_kb, int64_t n_rows, double *p_out_dev, int64_t n_ldo)
{
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		if(!p_a_dev || !p_b_dev || !p_out_dev || n_rows < 0)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "gram: null pointer or negative length");
		if(n_ka < 1 || n_ka > SLAMPP_HIP_GRAM_MAX_COLUMNS || n_kb < 1 || n_kb > SLAMPP_HIP_GRAM_MAX_COLUMNS)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "gram: between 1 and SLAMPP_HIP_GRAM_MAX_COLUMNS columns of a and of b");
		if((n_ka > 1 && n_lda < n_rows) || (n_kb > 1 && n_ldb < n_rows))
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "gram: the columns of a or b overlap (leading dimension below n_rows)");
		if(n_ldo < n_ka)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "gram: the columns of out overlap (leading dimension below n_ka)");
		const int64_t n_out_span = int64_t(n_kb - 1) * n_ldo + n_ka;
		if(ranges_overlap(p_a_dev, int64_t(n_ka - 1) * n_lda + n_rows, p_out_dev, n_out_span) ||
		   ranges_overlap(p_b_dev, int64_t(n_kb - 1) * n_ldb + n_rows, p_out_dev, n_out_span))
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "gram: out overlaps a or b");
		if(s.b_group_active)
			return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, "gram: this handle solves with landmark shards on several devices");
		s.d_gram.Alloc(gram_PARTIAL_DOUBLES);
		gram_enqueue(p_a_dev, n_lda, n_ka, p_b_dev, n_ldb, n_kb, n_rows, s.d_gram.p(), p_out_dev, n_ldo, s.stream);
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_refine_device_async(slampp_hip_solver *p_solver, const double *p_values_dev, const double *p_eta_dev,
	double *p_x_inout_dev, int n_steps, double *p_resid_inf_dev)
{
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		int n_check = multiply_checks(p_solver, "refine"), n_source = 0;
		if(n_check != SLAMPP_HIP_OK || (n_check = resolve_checks(p_solver, "refine", &n_source)) != SLAMPP_HIP_OK)
			return n_check;
		if(!p_values_dev || !p_eta_dev || !p_x_inout_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "refine: null pointer");
		if(n_steps < 1 || n_steps > 8)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "refine: between 1 and 8 steps");
		if(p_eta_dev == p_x_inout_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "refine: eta and x must be different vectors");
		s.Require_Multiply();
		s.d_refine_r.Alloc(2 * size_t(s.n_scalars)); // the one workspace: the residual, then the correction | the x before the step
		s.d_reduce.Alloc(reduce_MAX_PARTIALS);
		s.d_refine_resid.Alloc(refine_SCALARS);
		double *p_r = s.d_refine_r.p(), *p_keep = p_r + s.n_scalars;
		double *p_norm = (p_resid_inf_dev)? p_resid_inf_dev : s.d_refine_resid.p(); // (the norms decide, asked for or not)
		double *p_trial = s.d_refine_resid.p() + refine_TRIAL, *p_stop = s.d_refine_resid.p() + refine_STOP;
		const size_t n_bytes = size_t(s.n_scalars) * sizeof(double);
		SLAMPP_HIP_CHECK(hipMemsetAsync(p_stop, 0, sizeof(double), s.stream));
		for(int k = 0; k <= n_steps; ++ k) {
			SLAMPP_HIP_CHECK(hipMemcpyAsync(p_r, p_eta_dev, n_bytes, hipMemcpyDeviceToDevice, s.stream));
			multiply_enqueue(*s.p_mul, p_values_dev, p_x_inout_dev, p_r, -1.0, 1.0, s.stream); // r = eta - Lambda x
			norm_inf_enqueue(p_r, s.n_scalars, s.d_reduce.p(), (k)? p_trial : p_norm, s.stream);
			if(k) { // was step k - 1 worth taking? if not, x is put back and the steps after it add nothing
				refine_accept_enqueue(p_x_inout_dev, p_keep, s.n_scalars, p_norm + (k - 1), p_trial, p_norm + k, p_stop,
					s.stream);
			}
			if(k == n_steps)
				break;
			resolve_enqueue(s, p_r, n_source); // d = Lambda^-1 r with the kept factor
			refine_step_enqueue(p_x_inout_dev, p_keep, p_r, s.n_scalars, p_stop, s.stream);
		}
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_refine(slampp_hip_solver *p_solver, const double *p_values, const double *p_eta, double *p_x_inout, int n_steps,
	double *p_resid_inf)
{
	return host_round_trip(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		int n_check = multiply_checks(p_solver, "refine"), n_source = 0;
		if(n_check != SLAMPP_HIP_OK || (n_check = resolve_checks(p_solver, "refine", &n_source)) != SLAMPP_HIP_OK)
			return n_check;
		if(!p_values || !p_eta || !p_x_inout)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "refine: null pointer");
		if(n_steps < 1 || n_steps > 8)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "refine: between 1 and 8 steps");
		const size_t n_bytes = size_t(s.n_scalars) * sizeof(double);
		s.d_A.Alloc(size_t(s.n_values));
		s.d_mul_x.Alloc(size_t(s.n_scalars));
		s.d_mul_y.Alloc(size_t(s.n_scalars));
		s.d_refine_resid.Alloc(refine_SCALARS);
		Upload_Values_And_Join(s, p_values);
		SLAMPP_HIP_CHECK(hipMemcpyAsync(s.d_mul_y.p(), p_eta, n_bytes, hipMemcpyHostToDevice, s.stream));
		SLAMPP_HIP_CHECK(hipMemcpyAsync(s.d_mul_x.p(), p_x_inout, n_bytes, hipMemcpyHostToDevice, s.stream));
		return SLAMPP_HIP_OK;
	}, [&](slampp_hip_solver &s) {
		return slampp_hip_refine_device_async(p_solver, s.d_A.p(), s.d_mul_y.p(), s.d_mul_x.p(), n_steps,
			p_resid_inf? s.d_refine_resid.p() : 0);
	}, false, [&](slampp_hip_solver &s) {
		SLAMPP_HIP_CHECK(hipMemcpyAsync(p_x_inout, s.d_mul_x.p(), size_t(s.n_scalars) * sizeof(double), hipMemcpyDeviceToHost, s.stream));
		if(p_resid_inf)
			SLAMPP_HIP_CHECK(hipMemcpyAsync(p_resid_inf, s.d_refine_resid.p(), size_t(n_steps + 1) * sizeof(double), hipMemcpyDeviceToHost, s.stream));
	});
}

} // extern "C"
