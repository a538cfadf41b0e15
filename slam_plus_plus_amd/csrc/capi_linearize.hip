// capi_linearize.hip -- the C ABI of linearize.hip: slampp_hip_linearize_device_async, slampp_hip_state_plus_device_async and
// slampp_hip_chi_squared_device_async.  Every refusal is made on the host before anything is enqueued, with its text in
// slampp_hip_last_error under the names "linearize", "state_plus" and "chi2".
#include "capi_util.h"
#include "linearize.h"
#include "multiply.h"

using namespace slampp;

namespace {

// [a, a + n) and [b, b + n) share an element without being the same array
bool overlap_in_part(const double *p_a, const double *p_b, int64_t n)
{
	return p_a != p_b && p_a < p_b + n && p_b < p_a + n;
}

} // anonymous namespace

int slampp_hip_linearize_device_async(slampp_hip_assembly *p_assembly, int n_edge_type, const double *p_state_dev,
	const double *p_measurement_dev, const double *p_params_dev, double *p_J0_dev, double *p_J1_dev, double *p_error_dev)
{
	if(!p_assembly || !p_assembly->p_solver)
		return SLAMPP_HIP_ERR_INVALID; // (the solver it was created from is gone: nowhere to leave a text)
	slampp_hip_solver *p_solver = p_assembly->p_solver;
	return guarded(p_solver, [&]() -> int {
		if(p_assembly->b_stale)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "linearize: set_structure was called after this assembly was created");
		if(!p_state_dev || !p_measurement_dev || !p_J0_dev || !p_J1_dev || !p_error_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "linearize: null pointer");
		const TEdgeTypeShape t_shape = edge_type_shape(n_edge_type);
		if(!t_shape.b_known)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "linearize: unknown edge type");
		TAsmEdgeView t_edges;
		assembly_edge_view(*p_assembly->p_state, t_edges);
		if(t_edges.d0 != t_shape.d0 || t_edges.d1 != t_shape.d1 || t_edges.rd != t_shape.rd)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "linearize: the edge type's dimensions are not this assembly's");
		if(t_shape.n_params && !p_params_dev) {
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, (n_edge_type == SLAMPP_HIP_EDGE_P2C_XYZ)?
				"linearize: SLAMPP_HIP_EDGE_P2C_XYZ needs p_params_dev" : "linearize: SLAMPP_HIP_EDGE_P2SC_XYZ needs p_params_dev");
		}
		linearize_enqueue(n_edge_type, t_edges, p_state_dev, p_measurement_dev, p_params_dev, p_J0_dev, p_J1_dev, p_error_dev,
			p_solver->stream);
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_state_plus_device_async(slampp_hip_solver *p_solver, int n_vertex_type, int64_t n_first_vertex,
	int64_t n_last_vertex, const double *p_state_dev, const double *p_dx_dev, double f_scale, double *p_state_out_dev)
{
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		if(!s.b_has_structure)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "state_plus: set_structure was not called");
		if(!p_state_dev || !p_dx_dev || !p_state_out_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "state_plus: null pointer");
		int n_dim; // 0: any up to 8
		switch(n_vertex_type) {
		case SLAMPP_HIP_VERTEX_EUCLIDEAN: n_dim = 0; break;
		case SLAMPP_HIP_VERTEX_SE2: n_dim = 3; break;
		case SLAMPP_HIP_VERTEX_SE3: n_dim = 6; break;
		default: return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "state_plus: unknown vertex type");
		}
		const int64_t n = int64_t(s.cumsum.size()) - 1;
		if(n_first_vertex < 0 || n_first_vertex > n_last_vertex || n_last_vertex > n)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "state_plus: bad vertex range");
		for(int64_t v = n_first_vertex; v < n_last_vertex; ++ v) {
			const int64_t d = s.cumsum[v + 1] - s.cumsum[v];
			if((n_dim)? d != n_dim : d > 8)
				return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "state_plus: a block column in the range does not have the vertex type's dimension");
		}
		if(overlap_in_part(p_state_dev, p_state_out_dev, s.n_scalars) || overlap_in_part(p_dx_dev, p_state_out_dev, s.n_scalars) ||
		   p_dx_dev == p_state_out_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "state_plus: the state arrays overlap in part");
		if(!s.b_state_cumsum_valid) {
			s.d_state_cumsum.Upload(s.cumsum, s.stream);
			SLAMPP_HIP_CHECK(hipStreamSynchronize(s.stream)); // (set_structure may replace the host vector any time after)
			s.b_state_cumsum_valid = true;
		}
		state_plus_enqueue(n_vertex_type, s.d_state_cumsum.p(), n_first_vertex, n_last_vertex, p_state_dev, p_dx_dev, f_scale,
			p_state_out_dev, s.stream);
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_chi_squared_device_async(slampp_hip_assembly *p_assembly, const double *p_sigma_inv_dev, const double *p_error_dev,
	const double *p_weight_dev, double *p_out_dev)
{
	if(!p_assembly || !p_assembly->p_solver)
		return SLAMPP_HIP_ERR_INVALID;
	slampp_hip_solver *p_solver = p_assembly->p_solver;
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		if(p_assembly->b_stale)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "chi2: set_structure was called after this assembly was created");
		if(!p_sigma_inv_dev || !p_error_dev || !p_out_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "chi2: null pointer");
		TAsmEdgeView t_edges;
		assembly_edge_view(*p_assembly->p_state, t_edges);
		s.d_reduce.Alloc(reduce_MAX_PARTIALS);
		chi2_enqueue(t_edges.n_edges, t_edges.rd, p_sigma_inv_dev, p_error_dev, p_weight_dev, s.d_reduce.p(), p_out_dev, s.stream);
		return SLAMPP_HIP_OK;
	});
}
