// capi_covariance.hip -- the covariance entry points of the C ABI (include/slampp_hip.h): block-diagonal marginals, Lambda^-1 on
// Lambda's pattern, whole block columns of it and its blocks at arbitrary pairs, in the sparse mode and in the Schur mode, and
// the landmark-only solve
#include "capi_util.h"
#include "sparse_inverse.h"
#include "covariance.h"

#include <algorithm>

using namespace slampp;

extern "C" {

int slampp_hip_solve_marginal_poses_device_async(slampp_hip_solver *p_solver, const double *p_values_dev,
	double *p_rhs_inout_dev)
{
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		if(!s.b_analyzed)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "solve_marginal_poses: analyze was not called");
		if(s.n_mode != SLAMPP_HIP_MODE_SCHUR)
			return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, "solve_marginal_poses: needs the Schur mode (cameras and landmarks)");
		if(s.b_group_active)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "solve_marginal_poses_device: this handle solves with landmark shards on several devices: host entry points only");
		if(!p_values_dev || !p_rhs_inout_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "solve_marginal_poses: null pointer");
		schur_enqueue_marginal_poses(s, p_values_dev, p_rhs_inout_dev);
		s.Factor_Dropped(); // no factor of the reduced system comes out of this
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_solve_marginal_poses(slampp_hip_solver *p_solver, const double *p_values, double *p_rhs_inout)
{
	bool b_handed_over = false;
	return host_round_trip(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		if(!s.b_analyzed)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "solve_marginal_poses: analyze was not called");
		if(!p_values || !p_rhs_inout)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "solve_marginal_poses: null pointer");
		if((b_handed_over = s.b_group_active))
			return group_solve_marginal_poses(s, p_values, p_rhs_inout);
		s.d_A.Alloc(size_t(s.n_values));
		s.d_rhs.Alloc(size_t(s.n_scalars));
		s.Upload_Values(p_values);
		Upload_Rhs_And_Join(s, p_rhs_inout);
		return SLAMPP_HIP_OK;
	}, [&](slampp_hip_solver &s) {
		return slampp_hip_solve_marginal_poses_device_async(p_solver, s.d_A.p(), s.d_rhs.p());
	}, true, [&](slampp_hip_solver &s) {
		SLAMPP_HIP_CHECK(hipMemcpyAsync(p_rhs_inout, s.d_rhs.p(), size_t(s.n_scalars) * sizeof(double), hipMemcpyDeviceToHost, s.stream));
	}, &b_handed_over);
}

namespace {

// The numeric factorization of the sparse block path alone: the fused forward substitution reads a right-hand side, and
// with a dense top it rides through that factorization as a row of the matrix: zeros (a NaN there would spread through
// 0 x NaN in the tile products).  Inside guarded().
void factor_on_zeros(slampp_hip_solver &s, const double *p_values_dev)
{
	s.d_rhs.Alloc(size_t(s.n_scalars));
	SLAMPP_HIP_CHECK(hipMemsetAsync(s.d_rhs.p(), 0, size_t(s.n_scalars) * sizeof(double), s.stream));
	s.b_leaf_linv_wanted = true; // (the covariances multiply by inv(L_jj) of every column)
	// (with a dense top the whole factor + solve runs: the top is factored on the way; opens its own phases)
	s.Enqueue_Sparse(p_values_dev, s.d_rhs.p(), true, s.n_dense_dim == 0);
}

// what slampp_hip_marginals and slampp_hip_marginals_pattern share: the numeric factorization and the sparse inverse
// subset Z on the factor's pattern (d_Z; the dense top's part in d_Zd).  Inside guarded(), behind the caller's checks.
int enqueue_sparse_inverse(slampp_hip_solver *p_solver, const double *p_values_dev, const char *p_s_name)
{
	slampp_hip_solver &s = *p_solver;
	const Plan &P = s.plan;
	if(!s.b_sinv_tried) {
		s.b_sinv_tried = true;
		s.p_sinv = sparse_inverse_setup(P, s.stream, true);
		if(s.p_sinv) {
			std::vector<int64_t> zoff(size_t(P.n));
			for(int32_t c = 0; c < P.n; ++ c) {
				const int32_t j = P.pinv[c];
				zoff[c] = (P.dense_dim && P.dense_pos[j] >= 0)? -int64_t(P.dense_pos[j]) - 1 : P.loff[P.lptr[j]];
			}
			s.d_diag_zoff.Upload(zoff, s.stream);
			if(!P.uniform_dim) { // mixed block sizes: where every caller's column's block goes, and how big it is
				std::vector<int32_t> dims(size_t(P.n));
				std::vector<int64_t> out_off(size_t(P.n));
				int64_t n_at = 0;
				for(int32_t c = 0; c < P.n; ++ c) {
					dims[c] = int32_t(s.cumsum[c + 1] - s.cumsum[c]);
					out_off[c] = n_at;
					n_at += int64_t(dims[c]) * dims[c];
				}
				s.d_diag_dim.Upload(dims, s.stream);
				s.d_diag_out_off.Upload(out_off, s.stream);
			}
			s.d_Z.Alloc(size_t(P.loff.back()));
			if(s.n_dense_dim) {
				s.d_Zd.Alloc(size_t(s.n_dense_pad) * s.n_dense_pad);
				s.d_Zd_work.Alloc(size_t(s.n_dense_pad) * s.n_dense_pad);
			}
			SLAMPP_HIP_CHECK(hipStreamSynchronize(s.stream)); // zoff lives on this stack frame
		}
	}
	if(!s.p_sinv)
		return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, (std::string(p_s_name) + ": mixed block sizes are taken without a dense top only (set the option dense_top_nb to 0), block sizes above 8 not at all").c_str());
	s.b_leaf_linv_wanted = true; // (the inverse subset multiplies by inv(L_jj) of every column)
	if(p_values_dev) // (null: the factor in place -- the Schur covariance calls on a handle that went to this path)
		factor_on_zeros(s, p_values_dev);
	s.Ensure_Leaf_Inverses();
	s.Phase_Begin("marginals_inverse");
	if(s.n_dense_dim) { // the top's inverse from a copy of its factor (the factor itself stays for solve_again)
		SLAMPP_HIP_CHECK(hipMemcpyAsync(s.d_Zd_work.p(), s.d_dense.p(), size_t(s.n_dense_pad) * s.n_dense_pad * sizeof(double),
			hipMemcpyDeviceToDevice, s.stream));
		dense_top_clear_rhs_row(s.d_Zd_work.p(), s.n_dense_pad, s.stream);
		dense_inverse_from_factor(s.d_Zd_work.p(), s.n_dense_pad, s.d_dense_invdiag.p(), s.d_Zd.p(), s.stream);
	}
	sparse_inverse_enqueue(*s.p_sinv, P, s.d_L.p(), s.d_Linv.p(), s.d_Z.p(), s.stream, s.d_Zd.p(), s.n_dense_pad);
	s.Phase_End();
	return SLAMPP_HIP_OK;
}

} // anonymous namespace

int slampp_hip_marginals_device_async(slampp_hip_solver *p_solver, const double *p_values_dev, double *p_block_diag_dev)
{
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		if(!s.b_analyzed)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "marginals: analyze was not called");
		if(s.n_mode != SLAMPP_HIP_MODE_SPARSE)
			return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, "marginals: sparse mode only (Schur mode: slampp_hip_schur_marginals)");
		if(s.b_refined)
			return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, "marginals: block columns wider than 8 are factored in pieces: no covariance blocks in the caller's layout");
		if(!p_values_dev || !p_block_diag_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "marginals: null pointer");
		const int n_result = enqueue_sparse_inverse(p_solver, p_values_dev, "marginals");
		if(n_result != SLAMPP_HIP_OK)
			return n_result;
		const Plan &P = s.plan;
		if(P.uniform_dim)
			inverse_diag_blocks_launch(P.n, P.max_dim, s.d_diag_zoff.p(), s.d_Z.p(), s.d_Zd.p(), s.n_dense_pad, p_block_diag_dev, s.stream);
		else
			inverse_diag_blocks_any_launch(P.n, s.d_diag_dim.p(), s.d_diag_zoff.p(), s.d_diag_out_off.p(), s.d_Z.p(), p_block_diag_dev, s.stream);
		SLAMPP_HIP_CHECK(hipGetLastError());
		s.Factor_Installed(); // the factor of these values is in place
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_marginals(slampp_hip_solver *p_solver, const double *p_values, double *p_block_diag)
{
	size_t n_out = 0;
	return host_round_trip(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		if(!s.b_analyzed)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "marginals: analyze was not called");
		if(!p_values || !p_block_diag)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "marginals: null pointer");
		for(size_t c = 0; c + 1 < s.cumsum.size(); ++ c)
			n_out += size_t((s.cumsum[c + 1] - s.cumsum[c]) * (s.cumsum[c + 1] - s.cumsum[c]));
		s.d_A.Alloc(size_t(s.n_values));
		s.d_cov.Alloc(n_out);
		Upload_Values_And_Join(s, p_values);
		return SLAMPP_HIP_OK;
	}, [&](slampp_hip_solver &s) {
		return slampp_hip_marginals_device_async(p_solver, s.d_A.p(), s.d_cov.p());
	}, true, [&](slampp_hip_solver &s) {
		SLAMPP_HIP_CHECK(hipMemcpyAsync(p_block_diag, s.d_cov.p(), n_out * sizeof(double), hipMemcpyDeviceToHost, s.stream));
	});
}

namespace {

// the checks the covariance calls beyond the block diagonal share (inside guarded())
int covariance_checks(slampp_hip_solver *p_solver, const char *p_s_name)
{
	slampp_hip_solver &s = *p_solver;
	const std::string s_name(p_s_name);
	if(!s.b_analyzed)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, (s_name + ": analyze was not called").c_str());
	if(s.n_mode != SLAMPP_HIP_MODE_SPARSE)
		return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, (s_name + ": sparse mode only (Schur mode: slampp_hip_schur_marginals)").c_str());
	if(!s.group_devices.empty())
		return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, (s_name + ": not for a handle over several devices").c_str());
	if(s.b_refined)
		return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, (s_name + ": block columns wider than 8 are factored in pieces: no covariance blocks in the caller's layout").c_str());
	return SLAMPP_HIP_OK;
}

// n_cols distinct block columns in range; their scalar count in *p_k
int columns_checks(slampp_hip_solver *p_solver, int n_cols, const int64_t *p_bcols, int64_t *p_k)
{
	slampp_hip_solver &s = *p_solver;
	if(n_cols <= 0 || !p_bcols)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "marginal_columns: no columns");
	const int64_t n_bcols = int64_t(s.cumsum.size()) - 1;
	std::vector<int64_t> sorted(p_bcols, p_bcols + n_cols);
	std::sort(sorted.begin(), sorted.end());
	if(sorted.front() < 0 || sorted.back() >= n_bcols)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "marginal_columns: block column index out of range");
	if(std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "marginal_columns: a block column is listed twice");
	*p_k = 0;
	for(int i = 0; i < n_cols; ++ i)
		*p_k += s.cumsum[size_t(p_bcols[i] + 1)] - s.cumsum[size_t(p_bcols[i])];
	return SLAMPP_HIP_OK;
}

// n_pairs pairs of block columns in range; the doubles of their blocks in *p_n_out
int pairs_checks(slampp_hip_solver *p_solver, const char *p_s_name, int64_t n_pairs, const int64_t *p_brows, const int64_t *p_bcols,
	size_t *p_n_out)
{
	slampp_hip_solver &s = *p_solver;
	const std::string s_name(p_s_name);
	if(n_pairs <= 0 || !p_brows || !p_bcols)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, (s_name + ": no pairs").c_str());
	const int64_t n_bcols = int64_t(s.cumsum.size()) - 1;
	*p_n_out = 0;
	for(int64_t k = 0; k < n_pairs; ++ k) {
		const int64_t r = p_brows[k], c = p_bcols[k];
		if(r < 0 || r >= n_bcols || c < 0 || c >= n_bcols)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, (s_name + ": block column index out of range").c_str());
		*p_n_out += size_t((s.cumsum[size_t(r + 1)] - s.cumsum[size_t(r)]) * (s.cumsum[size_t(c + 1)] - s.cumsum[size_t(c)]));
	}
	return SLAMPP_HIP_OK;
}

// what the two marginal_blocks entry points check (inside guarded())
int marginal_blocks_checks(slampp_hip_solver *p_solver, bool b_values, int64_t n_pairs, const int64_t *p_brows,
	const int64_t *p_bcols, const double *p_out, size_t *p_n_out)
{
	int n_result = covariance_checks(p_solver, "marginal_blocks");
	if(n_result != SLAMPP_HIP_OK)
		return n_result;
	if(!p_out)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "marginal_blocks: null pointer");
	if((n_result = pairs_checks(p_solver, "marginal_blocks", n_pairs, p_brows, p_bcols, p_n_out)) != SLAMPP_HIP_OK)
		return n_result;
	if(!b_values && !p_solver->b_factored)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "marginal_blocks: no valid factorization to reuse (values = NULL)");
	return SLAMPP_HIP_OK;
}

// what slampp_hip_marginals_pattern_device_async does behind its checks (inside guarded()); p_values_dev = 0, which only
// the Schur covariance calls of a handle that went to the sparse path pass: the factor in place
int marginals_pattern_enqueue(slampp_hip_solver *p_solver, const double *p_values_dev, double *p_cov_dev, const char *p_s_name)
{
	slampp_hip_solver &s = *p_solver;
	const int n_result = enqueue_sparse_inverse(p_solver, p_values_dev, p_s_name);
	if(n_result != SLAMPP_HIP_OK)
		return n_result;
	covariance_pattern_enqueue(s, p_cov_dev);
	if(p_values_dev)
		s.Factor_Installed(); // the factor of these values is in place
	return SLAMPP_HIP_OK;
}

// the factor the substitutions of marginal_columns and marginal_blocks work from (inside guarded()); p_values_dev = 0: the
// factor in place, which the caller has found valid
void substitution_factor_enqueue(slampp_hip_solver &s, const double *p_values_dev)
{
	if(p_values_dev) { // factor these values (the fused forward substitution runs on zeros)
		factor_on_zeros(s, p_values_dev);
		s.Factor_Installed();
	}
	s.Ensure_Leaf_Inverses(); // (the substitutions multiply by inv(L_jj) of every column)
}

// what slampp_hip_marginal_columns_device_async does behind its checks (inside guarded())
void marginal_columns_enqueue(slampp_hip_solver &s, const double *p_values_dev, int n_cols, const int64_t *p_bcols, double *p_out_dev)
{
	substitution_factor_enqueue(s, p_values_dev);
	covariance_columns_enqueue(s, n_cols, p_bcols, p_out_dev);
}

// The second half of slampp_hip_marginal_columns and of its Schur twin, behind their checks and the upload of the values
// (b_values: into d_A): groups of whole block columns of at most COV_K_PASS scalar columns, each brought back behind its
// pass -- the device holds n_scalars x COV_K_PASS of the result (d_cov) at a time, whatever k is.  The first group factors
// the values, the others use that factor (values = NULL).
int marginal_columns_in_groups(slampp_hip_solver *p_solver, bool b_values, int n_cols, const int64_t *p_bcols, double *p_out,
	int (*p_device_async)(slampp_hip_solver*, const double*, int, const int64_t*, double*))
{
	slampp_hip_solver &s = *p_solver;
	const double *p_values_dev = b_values? s.d_A.p() : 0;
	int n_result = SLAMPP_HIP_OK;
	int64_t n_done = 0;
	for(int i = 0; i < n_cols && n_result == SLAMPP_HIP_OK;) {
		int n_group = 0;
		int64_t n_group_k = 0;
		while(i + n_group < n_cols) {
			const int64_t c = p_bcols[i + n_group], d = s.cumsum[size_t(c + 1)] - s.cumsum[size_t(c)];
			if(n_group && n_group_k + d > COV_K_PASS)
				break;
			n_group_k += d;
			++ n_group;
		}
		n_result = device_round_trip(p_solver, [&](slampp_hip_solver&) {
			return (*p_device_async)(p_solver, p_values_dev, n_group, p_bcols + i, s.d_cov.p());
		}, true, [&](slampp_hip_solver&) {
			SLAMPP_HIP_CHECK(hipMemcpyAsync(p_out + size_t(n_done) * size_t(s.n_scalars), s.d_cov.p(), size_t(n_group_k) *
				size_t(s.n_scalars) * sizeof(double), hipMemcpyDeviceToHost, s.stream));
		});
		p_values_dev = 0; // (the next groups reuse this factor)
		n_done += n_group_k;
		i += n_group;
	}
	return n_result;
}

} // anonymous namespace

int slampp_hip_marginals_pattern_device_async(slampp_hip_solver *p_solver, const double *p_values_dev, double *p_cov_dev)
{
	return guarded(p_solver, [&]() -> int {
		const int n_result = covariance_checks(p_solver, "marginals_pattern");
		if(n_result != SLAMPP_HIP_OK)
			return n_result;
		if(!p_values_dev || !p_cov_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "marginals_pattern: null pointer");
		return marginals_pattern_enqueue(p_solver, p_values_dev, p_cov_dev, "marginals_pattern");
	});
}

int slampp_hip_marginals_pattern(slampp_hip_solver *p_solver, const double *p_values, double *p_cov)
{
	return host_round_trip(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		const int n_check = covariance_checks(p_solver, "marginals_pattern");
		if(n_check != SLAMPP_HIP_OK)
			return n_check;
		if(!p_values || !p_cov)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "marginals_pattern: null pointer");
		s.d_A.Alloc(size_t(s.n_values));
		s.d_cov.Alloc(size_t(s.n_values));
		Upload_Values_And_Join(s, p_values);
		return SLAMPP_HIP_OK;
	}, [&](slampp_hip_solver &s) {
		return slampp_hip_marginals_pattern_device_async(p_solver, s.d_A.p(), s.d_cov.p());
	}, true, [&](slampp_hip_solver &s) {
		SLAMPP_HIP_CHECK(hipMemcpyAsync(p_cov, s.d_cov.p(), size_t(s.n_values) * sizeof(double), hipMemcpyDeviceToHost, s.stream));
	});
}

int slampp_hip_marginal_columns_device_async(slampp_hip_solver *p_solver, const double *p_values_dev, int n_cols,
	const int64_t *p_bcols, double *p_out_dev)
{
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		int n_result = covariance_checks(p_solver, "marginal_columns");
		if(n_result != SLAMPP_HIP_OK)
			return n_result;
		if(!p_out_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "marginal_columns: null pointer");
		int64_t n_k = 0;
		if((n_result = columns_checks(p_solver, n_cols, p_bcols, &n_k)) != SLAMPP_HIP_OK)
			return n_result;
		if(!p_values_dev && !s.b_factored)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "marginal_columns: no valid factorization to reuse (values = NULL)");
		marginal_columns_enqueue(s, p_values_dev, n_cols, p_bcols, p_out_dev);
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_marginal_columns(slampp_hip_solver *p_solver, const double *p_values, int n_cols, const int64_t *p_bcols,
	double *p_out)
{
	const int n_result = guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		int n_check = covariance_checks(p_solver, "marginal_columns");
		if(n_check != SLAMPP_HIP_OK)
			return n_check;
		if(!p_out)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "marginal_columns: null pointer");
		int64_t n_k = 0;
		if((n_check = columns_checks(p_solver, n_cols, p_bcols, &n_k)) != SLAMPP_HIP_OK)
			return n_check;
		if(!p_values && !s.b_factored)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "marginal_columns: no valid factorization to reuse (values = NULL)");
		s.d_cov.Alloc(size_t(s.n_scalars) * COV_K_PASS);
		if(p_values) {
			s.d_A.Alloc(size_t(s.n_values));
			Upload_Values_And_Join(s, p_values);
		}
		return SLAMPP_HIP_OK;
	});
	if(n_result != SLAMPP_HIP_OK)
		return n_result;
	return marginal_columns_in_groups(p_solver, p_values != 0, n_cols, p_bcols, p_out, slampp_hip_marginal_columns_device_async);
}

int slampp_hip_marginal_blocks_device_async(slampp_hip_solver *p_solver, const double *p_values_dev, int64_t n_pairs,
	const int64_t *p_brows, const int64_t *p_bcols, double *p_out_dev)
{
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		size_t n_out = 0;
		const int n_result = marginal_blocks_checks(p_solver, p_values_dev != 0, n_pairs, p_brows, p_bcols, p_out_dev, &n_out);
		if(n_result != SLAMPP_HIP_OK)
			return n_result;
		substitution_factor_enqueue(s, p_values_dev);
		covariance_pairs_enqueue(s, n_pairs, p_brows, p_bcols, p_out_dev);
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_marginal_blocks(slampp_hip_solver *p_solver, const double *p_values, int64_t n_pairs, const int64_t *p_brows,
	const int64_t *p_bcols, double *p_out)
{
	size_t n_out = 0;
	return host_round_trip(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		const int n_check = marginal_blocks_checks(p_solver, p_values != 0, n_pairs, p_brows, p_bcols, p_out, &n_out);
		if(n_check != SLAMPP_HIP_OK)
			return n_check;
		s.d_cov.Alloc(n_out);
		if(p_values) {
			s.d_A.Alloc(size_t(s.n_values));
			Upload_Values_And_Join(s, p_values);
		}
		return SLAMPP_HIP_OK;
	}, [&](slampp_hip_solver &s) {
		return slampp_hip_marginal_blocks_device_async(p_solver, p_values? s.d_A.p() : 0, n_pairs, p_brows, p_bcols, s.d_cov.p());
	}, true, [&](slampp_hip_solver &s) {
		SLAMPP_HIP_CHECK(hipMemcpyAsync(p_out, s.d_cov.p(), n_out * sizeof(double), hipMemcpyDeviceToHost, s.stream));
	});
}

int slampp_hip_schur_marginals_device_async(slampp_hip_solver *p_solver, const double *p_values_dev,
	double *p_cam_cov_dev, double *p_point_cov_dev)
{
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		if(!s.b_analyzed)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "schur_marginals: analyze was not called");
		if(s.n_mode != SLAMPP_HIP_MODE_SCHUR)
			return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, "schur_marginals: needs the Schur mode (cameras and landmarks)");
		if(s.b_group_active)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "schur_marginals_device: this handle solves with landmark shards on several devices: host entry points only");
		if(!p_values_dev || (!p_cam_cov_dev && !p_point_cov_dev))
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "schur_marginals: null pointer");
		schur_enqueue_marginals(s, p_values_dev, p_cam_cov_dev, p_point_cov_dev);
		s.Factor_Dropped(); // C^-1 and W were recomputed from these values: a kept factor may no longer match them
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_schur_marginals(slampp_hip_solver *p_solver, const double *p_values, double *p_cam_cov, double *p_point_cov)
{
	size_t n_cam_doubles = 0, n_point_doubles = 0;
	bool b_handed_over = false;
	return host_round_trip(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		if(!s.b_analyzed)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "schur_marginals: analyze was not called");
		if(s.n_mode != SLAMPP_HIP_MODE_SCHUR)
			return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, "schur_marginals: needs the Schur mode (cameras and landmarks)");
		if(!p_values || (!p_cam_cov && !p_point_cov))
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "schur_marginals: null pointer");
		if((b_handed_over = s.b_group_active))
			return group_schur_marginals(s, p_values, p_cam_cov, p_point_cov);
		const int64_t nc = s.n_matrix_cut, np = int64_t(s.cumsum.size()) - 1 - nc;
		const int64_t dc = s.cumsum[1] - s.cumsum[0], dp = s.cumsum[nc + 1] - s.cumsum[nc];
		n_cam_doubles = size_t(nc * dc * dc);
		n_point_doubles = size_t(np * dp * dp);
		s.d_A.Alloc(size_t(s.n_values));
		s.d_cov.Alloc(n_cam_doubles + n_point_doubles);
		Upload_Values_And_Join(s, p_values);
		return SLAMPP_HIP_OK;
	}, [&](slampp_hip_solver &s) {
		return slampp_hip_schur_marginals_device_async(p_solver, s.d_A.p(), p_cam_cov? s.d_cov.p() : 0,
			p_point_cov? s.d_cov.p() + n_cam_doubles : 0);
	}, true, [&](slampp_hip_solver &s) {
		if(p_cam_cov)
			SLAMPP_HIP_CHECK(hipMemcpyAsync(p_cam_cov, s.d_cov.p(), n_cam_doubles * sizeof(double), hipMemcpyDeviceToHost, s.stream));
		if(p_point_cov)
			SLAMPP_HIP_CHECK(hipMemcpyAsync(p_point_cov, s.d_cov.p() + n_cam_doubles, n_point_doubles * sizeof(double),
				hipMemcpyDeviceToHost, s.stream));
	}, &b_handed_over);
}

namespace {

// the checks of the Schur covariance calls beyond the block diagonal (inside guarded()); *p_b_fallback: the handle went to
// the sparse path (its layouts are the same: the sparse calls answer).  b_reuse: values = NULL, which takes what the last
// of these calls left only if no other factorization ran since and that one was positive definite
int schur_cov_checks(slampp_hip_solver *p_solver, const char *p_s_name, bool b_reuse, bool *p_b_fallback)
{
	slampp_hip_solver &s = *p_solver;
	const std::string s_name(p_s_name);
	*p_b_fallback = false;
	if(!s.b_analyzed)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, (s_name + ": analyze was not called").c_str());
	if(s.b_group_active || !s.group_devices.empty())
		return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, (s_name + ": not for a handle over several devices").c_str());
	if(s.n_mode == SLAMPP_HIP_MODE_SPARSE && s.b_schur_fallback)
		*p_b_fallback = true;
	else if(s.n_mode != SLAMPP_HIP_MODE_SCHUR)
		return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, (s_name + ": needs the Schur mode (sparse mode: slampp_hip_marginals_pattern, slampp_hip_marginal_columns)").c_str());
	else if(s.p_allreduce)
		return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, (s_name + ": not with landmark shards (an all-reduce callback is set)").c_str());
	if(b_reuse && (!s.n_schur_cov_gen || s.n_schur_cov_gen != s.n_factor_gen))
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, (s_name + ": no factorization to reuse (values = NULL): none was left by a Schur covariance call, another factorization ran since, or it was not positive definite").c_str());
	return SLAMPP_HIP_OK;
}

// how a Schur covariance call leaves the handle (inside guarded()).  Schur mode: C^-1 and W were recomputed from these
// values, a kept factor may no longer match them; a handle that went to the sparse path has counted its factor in itself.
// values = NULL has factored nothing and counts nothing up: what it reused stays valid, for the next such call too
void schur_cov_done(slampp_hip_solver &s, bool b_values, bool b_fallback)
{
	if(b_values && !b_fallback)
		s.Factor_Dropped();
	s.Schur_Cov_Left();
}

} // anonymous namespace

int slampp_hip_schur_marginals_pattern_device_async(slampp_hip_solver *p_solver, const double *p_values_dev, double *p_cov_dev)
{
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		bool b_fallback = false;
		int n_result = schur_cov_checks(p_solver, "schur_marginals_pattern", !p_values_dev, &b_fallback);
		if(n_result != SLAMPP_HIP_OK)
			return n_result;
		if(!p_cov_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "schur_marginals_pattern: null pointer");
		if(b_fallback) { // what slampp_hip_marginals_pattern does
			if((n_result = covariance_checks(p_solver, "schur_marginals_pattern")) != SLAMPP_HIP_OK ||
			   (n_result = marginals_pattern_enqueue(p_solver, p_values_dev, p_cov_dev, "schur_marginals_pattern")) != SLAMPP_HIP_OK)
				return n_result;
		} else
			schur_cov_pattern_enqueue(s, p_values_dev, p_cov_dev);
		schur_cov_done(s, p_values_dev != 0, b_fallback);
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_schur_marginals_pattern(slampp_hip_solver *p_solver, const double *p_values, double *p_cov)
{
	return host_round_trip(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		bool b_fallback = false;
		const int n_check = schur_cov_checks(p_solver, "schur_marginals_pattern", !p_values, &b_fallback);
		if(n_check != SLAMPP_HIP_OK)
			return n_check;
		if(!p_cov)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "schur_marginals_pattern: null pointer");
		s.d_cov.Alloc(size_t(s.n_values));
		if(p_values) {
			s.d_A.Alloc(size_t(s.n_values));
			Upload_Values_And_Join(s, p_values);
		}
		return SLAMPP_HIP_OK;
	}, [&](slampp_hip_solver &s) {
		return slampp_hip_schur_marginals_pattern_device_async(p_solver, p_values? s.d_A.p() : 0, s.d_cov.p());
	}, true, [&](slampp_hip_solver &s) {
		SLAMPP_HIP_CHECK(hipMemcpyAsync(p_cov, s.d_cov.p(), size_t(s.n_values) * sizeof(double), hipMemcpyDeviceToHost, s.stream));
	});
}

int slampp_hip_schur_marginal_columns_device_async(slampp_hip_solver *p_solver, const double *p_values_dev, int n_cols,
	const int64_t *p_bcols, double *p_out_dev)
{
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		bool b_fallback = false;
		int n_result = schur_cov_checks(p_solver, "schur_marginal_columns", !p_values_dev, &b_fallback);
		if(n_result != SLAMPP_HIP_OK)
			return n_result;
		if(!p_out_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "schur_marginal_columns: null pointer");
		int64_t n_k = 0;
		if((n_result = columns_checks(p_solver, n_cols, p_bcols, &n_k)) != SLAMPP_HIP_OK)
			return n_result;
		if(b_fallback) { // what slampp_hip_marginal_columns does
			if((n_result = covariance_checks(p_solver, "schur_marginal_columns")) != SLAMPP_HIP_OK)
				return n_result;
			marginal_columns_enqueue(s, p_values_dev, n_cols, p_bcols, p_out_dev);
		} else
			schur_cov_columns_enqueue(s, p_values_dev, n_cols, p_bcols, p_out_dev);
		schur_cov_done(s, p_values_dev != 0, b_fallback);
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_schur_marginal_columns(slampp_hip_solver *p_solver, const double *p_values, int n_cols, const int64_t *p_bcols,
	double *p_out)
{
	const int n_result = guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		bool b_fallback = false;
		int n_check = schur_cov_checks(p_solver, "schur_marginal_columns", !p_values, &b_fallback);
		if(n_check != SLAMPP_HIP_OK)
			return n_check;
		if(!p_out)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "schur_marginal_columns: null pointer");
		int64_t n_k = 0;
		if((n_check = columns_checks(p_solver, n_cols, p_bcols, &n_k)) != SLAMPP_HIP_OK)
			return n_check;
		s.d_cov.Alloc(size_t(s.n_scalars) * COV_K_PASS);
		if(p_values) {
			s.d_A.Alloc(size_t(s.n_values));
			Upload_Values_And_Join(s, p_values);
		}
		return SLAMPP_HIP_OK;
	});
	if(n_result != SLAMPP_HIP_OK)
		return n_result;
	// (values = NULL for the groups behind the first: the generation check lets them through)
	return marginal_columns_in_groups(p_solver, p_values != 0, n_cols, p_bcols, p_out, slampp_hip_schur_marginal_columns_device_async);
}

namespace {

// what the two schur_marginal_blocks entry points check (inside guarded())
int schur_marginal_blocks_checks(slampp_hip_solver *p_solver, bool b_values, int64_t n_pairs, const int64_t *p_brows,
	const int64_t *p_bcols, const double *p_out, size_t *p_n_out, bool *p_b_fallback)
{
	int n_result = schur_cov_checks(p_solver, "schur_marginal_blocks", !b_values, p_b_fallback);
	if(n_result != SLAMPP_HIP_OK)
		return n_result;
	if(!p_out)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "schur_marginal_blocks: null pointer");
	if((n_result = pairs_checks(p_solver, "schur_marginal_blocks", n_pairs, p_brows, p_bcols, p_n_out)) != SLAMPP_HIP_OK)
		return n_result;
	if(*p_b_fallback) // what slampp_hip_marginal_blocks checks
		return covariance_checks(p_solver, "schur_marginal_blocks");
	return SLAMPP_HIP_OK;
}

} // anonymous namespace

int slampp_hip_schur_marginal_blocks_device_async(slampp_hip_solver *p_solver, const double *p_values_dev, int64_t n_pairs,
	const int64_t *p_brows, const int64_t *p_bcols, double *p_out_dev)
{
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		bool b_fallback = false;
		size_t n_out = 0;
		const int n_result = schur_marginal_blocks_checks(p_solver, p_values_dev != 0, n_pairs, p_brows, p_bcols, p_out_dev, &n_out,
			&b_fallback);
		if(n_result != SLAMPP_HIP_OK)
			return n_result;
		if(b_fallback) { // what slampp_hip_marginal_blocks does
			substitution_factor_enqueue(s, p_values_dev);
			covariance_pairs_enqueue(s, n_pairs, p_brows, p_bcols, p_out_dev);
		} else
			schur_cov_pairs_enqueue(s, p_values_dev, n_pairs, p_brows, p_bcols, p_out_dev);
		schur_cov_done(s, p_values_dev != 0, b_fallback);
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_schur_marginal_blocks(slampp_hip_solver *p_solver, const double *p_values, int64_t n_pairs, const int64_t *p_brows,
	const int64_t *p_bcols, double *p_out)
{
	size_t n_out = 0;
	return host_round_trip(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		bool b_fallback = false;
		const int n_check = schur_marginal_blocks_checks(p_solver, p_values != 0, n_pairs, p_brows, p_bcols, p_out, &n_out, &b_fallback);
		if(n_check != SLAMPP_HIP_OK)
			return n_check;
		s.d_cov.Alloc(n_out);
		if(p_values) {
			s.d_A.Alloc(size_t(s.n_values));
			Upload_Values_And_Join(s, p_values);
		}
		return SLAMPP_HIP_OK;
	}, [&](slampp_hip_solver &s) {
		return slampp_hip_schur_marginal_blocks_device_async(p_solver, p_values? s.d_A.p() : 0, n_pairs, p_brows, p_bcols, s.d_cov.p());
	}, true, [&](slampp_hip_solver &s) {
		SLAMPP_HIP_CHECK(hipMemcpyAsync(p_out, s.d_cov.p(), n_out * sizeof(double), hipMemcpyDeviceToHost, s.stream));
	});
}

} // extern "C"
