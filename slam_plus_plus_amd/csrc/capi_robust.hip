// capi_robust.hip -- the C ABI of robust.hip: slampp_hip_assembly_set_robust, slampp_hip_assembly_robust_weights and the three
// kernels' entry points.  Every refusal is made on the host before anything is enqueued, with its text in
// slampp_hip_last_error under the name "robust".
#include "capi_util.h"
#include "robust.h"
#include "multiply.h"

using namespace slampp;

namespace {

// a live handle that no set_structure has outdated, with a specification where one is needed (inside guarded())
int check_handle(slampp_hip_solver *p_solver, const slampp_hip_assembly *p_assembly, bool b_need_spec)
{
	if(p_assembly->b_stale)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "robust: set_structure was called after this assembly was created");
	if(b_need_spec && !p_assembly->b_robust)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "robust: no robust kernel is set on this assembly");
	return SLAMPP_HIP_OK;
}

} // anonymous namespace

int slampp_hip_assembly_set_robust(slampp_hip_assembly *p_assembly, const slampp_hip_robust *p_robust)
{
	if(!p_assembly || !p_assembly->p_solver)
		return SLAMPP_HIP_ERR_INVALID; // (the solver it was created from is gone: nowhere to leave a text)
	slampp_hip_solver *p_solver = p_assembly->p_solver;
	return guarded(p_solver, [&]() -> int {
		const int n_check = check_handle(p_solver, p_assembly, false);
		if(n_check != SLAMPP_HIP_OK)
			return n_check;
		if(!p_robust) {
			if(p_assembly->b_robust) {
				SLAMPP_HIP_CHECK(hipStreamSynchronize(p_solver->stream)); // (a kernel may still be writing the array)
				p_assembly->d_robust_weight.Release();
				p_assembly->b_robust = false;
			}
			return SLAMPP_HIP_OK;
		}
		const slampp_hip_robust &r = *p_robust;
		if(r.n_kernel != SLAMPP_HIP_ROBUST_HUBER && r.n_kernel != SLAMPP_HIP_ROBUST_CAUCHY && r.n_kernel != SLAMPP_HIP_ROBUST_TUKEY &&
		   r.n_kernel != SLAMPP_HIP_ROBUST_WELSCH)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "robust: unknown kernel");
		if(r.n_basis != SLAMPP_HIP_ROBUST_BASIS_ERROR_NORM && r.n_basis != SLAMPP_HIP_ROBUST_BASIS_CHI2 &&
		   r.n_basis != SLAMPP_HIP_ROBUST_BASIS_MAHALANOBIS)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "robust: unknown basis");
		if(r.n_mode != SLAMPP_HIP_ROBUST_MODE_REFERENCE && r.n_mode != SLAMPP_HIP_ROBUST_MODE_LOSS)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "robust: unknown mode");
		if(!(r.f_scale > 0) || !(r.f_param > 0)) // (a NaN is not positive)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "robust: the scale and the parameter must be positive");
		if(r.n_mode == SLAMPP_HIP_ROBUST_MODE_LOSS && r.n_basis != SLAMPP_HIP_ROBUST_BASIS_MAHALANOBIS)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "robust: SLAMPP_HIP_ROBUST_MODE_LOSS needs SLAMPP_HIP_ROBUST_BASIS_MAHALANOBIS");
		TAsmEdgeView t_edges;
		assembly_edge_view(*p_assembly->p_state, t_edges); // (rd <= 8, d0, d1 <= 7: slampp_hip_assembly_create saw to it)
		if(!p_assembly->b_robust)
			p_assembly->d_robust_weight.Alloc(size_t(t_edges.n_edges));
		p_assembly->t_robust = r;
		p_assembly->b_robust = true;
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_assembly_robust_weights(slampp_hip_assembly *p_assembly, const double **pp_weight_dev)
{
	if(pp_weight_dev)
		*pp_weight_dev = 0;
	if(!p_assembly || !p_assembly->p_solver)
		return SLAMPP_HIP_ERR_INVALID;
	slampp_hip_solver *p_solver = p_assembly->p_solver;
	return guarded(p_solver, [&]() -> int {
		if(!pp_weight_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "robust: null pointer");
		*pp_weight_dev = (p_assembly->b_robust)? p_assembly->d_robust_weight.p() : 0;
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_robust_weights_device_async(slampp_hip_assembly *p_assembly, const double *p_sigma_inv_dev, const double *p_error_dev,
	double *p_weight_out_dev)
{
	if(!p_assembly || !p_assembly->p_solver)
		return SLAMPP_HIP_ERR_INVALID;
	slampp_hip_solver *p_solver = p_assembly->p_solver;
	return guarded(p_solver, [&]() -> int {
		const int n_check = check_handle(p_solver, p_assembly, true);
		if(n_check != SLAMPP_HIP_OK)
			return n_check;
		const slampp_hip_robust &r = p_assembly->t_robust;
		if(!p_error_dev || (!p_sigma_inv_dev && r.n_basis != SLAMPP_HIP_ROBUST_BASIS_ERROR_NORM))
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "robust: null pointer");
		TAsmEdgeView t_edges;
		assembly_edge_view(*p_assembly->p_state, t_edges);
		robust_weights_enqueue(r, t_edges.n_edges, t_edges.rd, p_sigma_inv_dev, p_error_dev,
			(p_weight_out_dev)? p_weight_out_dev : p_assembly->d_robust_weight.p(), p_solver->stream);
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_robust_scale_device_async(slampp_hip_assembly *p_assembly, const double *p_weight_dev, double *p_J0_dev,
	double *p_J1_dev, double *p_error_dev)
{
	if(!p_assembly || !p_assembly->p_solver)
		return SLAMPP_HIP_ERR_INVALID;
	slampp_hip_solver *p_solver = p_assembly->p_solver;
	return guarded(p_solver, [&]() -> int {
		const int n_check = check_handle(p_solver, p_assembly, true);
		if(n_check != SLAMPP_HIP_OK)
			return n_check;
		if(!p_J0_dev || !p_J1_dev || !p_error_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "robust: null pointer");
		TAsmEdgeView t_edges;
		assembly_edge_view(*p_assembly->p_state, t_edges);
		robust_scale_enqueue(t_edges.n_edges, t_edges.rd, t_edges.d0, t_edges.d1,
			(p_weight_dev)? p_weight_dev : p_assembly->d_robust_weight.p(), p_J0_dev, p_J1_dev, p_error_dev, p_solver->stream);
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_robust_chi_squared_device_async(slampp_hip_assembly *p_assembly, const double *p_sigma_inv_dev,
	const double *p_error_dev, double *p_out_dev)
{
	if(!p_assembly || !p_assembly->p_solver)
		return SLAMPP_HIP_ERR_INVALID;
	slampp_hip_solver *p_solver = p_assembly->p_solver;
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		const int n_check = check_handle(p_solver, p_assembly, true);
		if(n_check != SLAMPP_HIP_OK)
			return n_check;
		if(p_assembly->t_robust.n_basis != SLAMPP_HIP_ROBUST_BASIS_MAHALANOBIS)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "robust: the robust cost needs SLAMPP_HIP_ROBUST_BASIS_MAHALANOBIS");
		if(!p_sigma_inv_dev || !p_error_dev || !p_out_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "robust: null pointer");
		TAsmEdgeView t_edges;
		assembly_edge_view(*p_assembly->p_state, t_edges);
		s.d_reduce.Alloc(reduce_MAX_PARTIALS);
		robust_chi2_enqueue(p_assembly->t_robust, t_edges.n_edges, t_edges.rd, p_sigma_inv_dev, p_error_dev, s.d_reduce.p(), p_out_dev,
			s.stream);
		return SLAMPP_HIP_OK;
	});
}
