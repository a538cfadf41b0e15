// capi_logdet.hip -- the entry points of the C ABI (include/slampp_hip.h) that give log det Lambda = 2 sum log L_ii from the
// Cholesky factor on the device (kernels: logdet.hip; where the pivots live: logdet_tables.h).  In Schur mode
// log det Lambda = log det S + sum over the landmarks of log det C_p, S the reduced camera system.
#include "capi_util.h"
#include "logdet.h"
#include "logdet_tables.h"
#include "multiply.h"
#include "schur_state.h"

#include <cmath>
#include <limits>

using namespace slampp;

// the pivot table of the current plan, built at the first log-determinant after an analysis
void slampp_hip_solver::Require_Logdet_Table()
{
	if(b_logdet_valid && d_logdet_tab.p())
		return;
	build_logdet_table(plan, logdet_tab_host);
	d_logdet_tab.Upload(logdet_tab_host, stream);
	b_logdet_valid = true;
}

namespace {

// the checks of both entry points (inside guarded()), decided before anything is uploaded or enqueued
int logdet_checks(slampp_hip_solver *p_solver, bool b_values, int b_reuse_factor, bool b_out)
{
	slampp_hip_solver &s = *p_solver;
	if(s.b_group_active || (s.n_mode == SLAMPP_HIP_MODE_SCHUR && s.p_allreduce))
		return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, "logdet: not for a handle that solves with landmark shards or over several devices");
	if(!s.b_analyzed)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "logdet: analyze was not called");
	if(!b_out)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "logdet: null pointer");
	if(!b_reuse_factor)
		return b_values? SLAMPP_HIP_OK : fail(p_solver, SLAMPP_HIP_ERR_INVALID, "logdet: null values (they are factored first)");
	if(s.n_mode == SLAMPP_HIP_MODE_SPARSE) // (a Schur handle whose analysis went to the sparse path is a sparse handle)
		return s.b_factored? SLAMPP_HIP_OK : fail(p_solver, SLAMPP_HIP_ERR_INVALID, "logdet: no valid factorization to reuse");
	if(!s.p_schur || !s.n_factor_gen || s.n_schur_keep_gen != s.n_factor_gen) {
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, (s.p_schur && s.n_factor_gen && s.n_schur_cov_gen == s.n_factor_gen)?
			"logdet: the factor in place is what a Schur covariance call left, whose dense route holds inv(L), not L: reuse "
			"needs a solve that kept its factor (option schur_keep or schur_incremental)" :
			"logdet: no kept factor of the reduced camera system to reuse: set the option schur_keep (or schur_incremental) "
			"before analyze and solve; anything that factors or fails to since ends its validity");
	}
	if(!b_values)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "logdet: null values (Schur mode reads the landmarks' blocks C_p from them)");
	return SLAMPP_HIP_OK;
}

} // anonymous namespace

extern "C" {

int slampp_hip_logdet_device_async(slampp_hip_solver *p_solver, const double *p_values_dev, int b_reuse_factor,
	double *p_logdet_dev)
{
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		const int n_check = logdet_checks(p_solver, p_values_dev != 0, b_reuse_factor, p_logdet_dev != 0);
		if(n_check != SLAMPP_HIP_OK)
			return n_check;
		const bool b_sparse = s.n_mode == SLAMPP_HIP_MODE_SPARSE;
		if(!b_reuse_factor) {
			// the numeric factorization, and the handle left as slampp_hip_factor_solve_device_async leaves it.  The factor
			// kernels carry a forward substitution along: it runs on zeros of the library's own.  Sparse mode without a dense
			// top stops behind the factor; with one, and in Schur mode, the shortest route that leaves a factor other
			// right-hand sides can be solved from is the solve itself (on zeros)
			s.d_rhs.Alloc(size_t(s.n_scalars));
			SLAMPP_HIP_CHECK(hipMemsetAsync(s.d_rhs.p(), 0, size_t(s.n_scalars) * sizeof(double), s.stream));
			if(b_sparse)
				s.Enqueue_Sparse(p_values_dev, s.d_rhs.p(), true, s.n_dense_dim == 0);
			else
				schur_enqueue(s, p_values_dev, s.d_rhs.p());
			s.Factor_Installed();
			if(!b_sparse && schur_keeps_for_resolve(s))
				s.Schur_Kept();
		}
		TLogdetSources t = {};
		if(b_sparse) {
			s.Require_Logdet_Table();
			t.p_table = s.d_logdet_tab.p();
			t.n_table = int64_t(s.logdet_tab_host.size());
			t.p_L = s.d_L.p();
			t.p_dense = s.d_dense.p();
			t.n_dense_ld = s.n_dense_pad;
		} else {
			CSchurState &S = *s.p_schur;
			if(!S.b_reduced_decided)
				return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "logdet: the reduced camera system has not been factored");
			if(S.b_reduced_sparse) { // S went through the sparse block path: the inner solver's pivots
				slampp_hip_solver &r_in = *S.p_inner;
				r_in.Require_Logdet_Table();
				t.p_table = r_in.d_logdet_tab.p();
				t.n_table = int64_t(r_in.logdet_tab_host.size());
				t.p_L = r_in.d_L.p();
				t.p_dense = r_in.d_dense.p();
				t.n_dense_ld = r_in.n_dense_pad;
			} else { // the diagonal of d_S, rows < N, after dense_cholesky
				t.p_diag = S.d_S.p();
				t.n_diag = S.N;
				t.n_diag_ld = S.Npad;
			}
			t.p_values = p_values_dev;
			t.p_ptr = S.d_ptr.p();
			t.n_cams = S.nc;
			t.n_points = S.np;
			t.n_dc = S.DC;
			t.n_dp = S.DP;
		}
		s.d_reduce.Alloc(reduce_MAX_PARTIALS + 1); // (the last one: the result of the host entry point)
		logdet_enqueue(t, s.d_reduce.p(), s.d_flag.p(), p_logdet_dev, s.stream);
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_logdet(slampp_hip_solver *p_solver, const double *p_values, int b_reuse_factor, double *p_logdet)
{
	if(p_logdet)
		*p_logdet = std::numeric_limits<double>::quiet_NaN(); // (what a matrix that is not positive definite leaves)
	return host_round_trip(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		const int n_check = logdet_checks(p_solver, p_values != 0, b_reuse_factor, p_logdet != 0);
		if(n_check != SLAMPP_HIP_OK)
			return n_check;
		s.d_reduce.Alloc(reduce_MAX_PARTIALS + 1);
		if(p_values && (!b_reuse_factor || s.n_mode != SLAMPP_HIP_MODE_SPARSE)) {
			s.d_A.Alloc(size_t(s.n_values));
			Upload_Values_And_Join(s, p_values);
		}
		return SLAMPP_HIP_OK;
	}, [&](slampp_hip_solver &s) {
		return slampp_hip_logdet_device_async(p_solver, s.d_A.p(), b_reuse_factor, s.d_reduce.p() + reduce_MAX_PARTIALS);
	}, true, [&](slampp_hip_solver &s) {
		SLAMPP_HIP_CHECK(hipMemcpyAsync(p_logdet, s.d_reduce.p() + reduce_MAX_PARTIALS, sizeof(double), hipMemcpyDeviceToHost, s.stream));
	});
}

} // extern "C"
