// capi_lm.hip -- the C ABI of lm.hip: the building blocks of a Levenberg-Marquardt loop that is decided on the device
// (slampp_hip_edge_errors_device_async, slampp_hip_apply_damping_scalar_device_async and the slampp_hip_lm_* calls) and the
// loop made of them (slampp_hip_lm_begin_device_async, slampp_hip_lm_iterate_device_async).  Every refusal is made on the host
// before anything is enqueued, with its text in slampp_hip_last_error under the name "lm".
#include "capi_util.h"
#include "linearize.h"
#include "lm.h"
#include "multiply.h"

#include <algorithm>

using namespace slampp;

namespace {

const char *p_s_sharded = "lm: not for a handle that solves with landmark shards or over several devices";

// [a, a + n) and [b, b + n) share an element
bool overlap(const double *p_a, const double *p_b, int64_t n)
{
	return p_a < p_b + n && p_b < p_a + n;
}

// an assembly handle of this solver that no set_structure has outdated, and an edge type of its dimensions (inside guarded())
int check_edge_set(slampp_hip_solver *p_solver, const slampp_hip_assembly *p_assembly, int n_edge_type, bool b_params)
{
	if(!p_assembly || p_assembly->p_solver != p_solver)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: an edge set's assembly is null or belongs to another solver");
	if(p_assembly->b_stale)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: set_structure was called after an assembly was created");
	const TEdgeTypeShape t_shape = edge_type_shape(n_edge_type);
	TAsmEdgeView t_edges;
	assembly_edge_view(*p_assembly->p_state, t_edges);
	if(!t_shape.b_known || t_edges.d0 != t_shape.d0 || t_edges.d1 != t_shape.d1 || t_edges.rd != t_shape.rd)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: an edge type does not fit its assembly");
	if(t_shape.n_params && !b_params)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: null pointer");
	return SLAMPP_HIP_OK;
}

// everything slampp_hip_lm_begin_device_async and slampp_hip_lm_iterate_device_async refuse (inside guarded())
int check_problem(const slampp_hip_lm_problem &r)
{
	slampp_hip_solver *p_solver = r.p_solver;
	slampp_hip_solver &s = *p_solver;
	if(s.b_group_active || s.p_allreduce)
		return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, p_s_sharded);
	if(!s.b_analyzed)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: analyze was not called");
	if(r.n_sets < 1 || r.n_sets > SLAMPP_HIP_LM_MAX_SETS)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: between 1 and SLAMPP_HIP_LM_MAX_SETS edge sets");
	if(!r.p_sets || !r.p_ranges || !r.p_state_dev || !r.p_trial_dev || !r.p_values_dev || !r.p_eta_dev || !r.p_dx_dev || !r.p_lm_dev ||
	   !r.p_chi_parts_dev || r.n_trace_capacity < 0)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: null pointer");
	for(int i = 0; i < r.n_sets; ++ i) {
		const slampp_hip_lm_edge_set &t = r.p_sets[i];
		const int n_check = check_edge_set(p_solver, t.p_assembly, t.n_edge_type, t.p_params_dev != 0);
		if(n_check != SLAMPP_HIP_OK)
			return n_check;
		if(!t.p_measurement_dev || !t.p_sigma_inv_dev || !t.p_J0_dev || !t.p_J1_dev || !t.p_error_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: null pointer");
		if(t.p_assembly->b_robust && t.p_weight_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: an edge set has both a robust kernel and a weight array");
	}
	const int64_t n = int64_t(s.cumsum.size()) - 1;
	if(r.n_unary_vertex < -1 || r.n_unary_vertex >= n)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: the unary vertex is not a block column");
	// the ranges in the order of their first block column: each begins where the one before it ended
	std::vector<int> order;
	for(int i = 0; i < r.n_ranges; ++ i) {
		const slampp_hip_lm_vertex_range &t = r.p_ranges[i];
		if(t.n_vertex_type != SLAMPP_HIP_VERTEX_EUCLIDEAN && t.n_vertex_type != SLAMPP_HIP_VERTEX_SE2 && t.n_vertex_type != SLAMPP_HIP_VERTEX_SE3)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: unknown vertex type");
		if(t.n_first_vertex < 0 || t.n_first_vertex > t.n_last_vertex)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: the vertex ranges do not cover the block columns exactly once");
		if(t.n_first_vertex < t.n_last_vertex) // (an empty range covers nothing)
			order.push_back(i);
	}
	std::sort(order.begin(), order.end(), [&](int a, int b) { return r.p_ranges[a].n_first_vertex < r.p_ranges[b].n_first_vertex; });
	int64_t n_covered = 0;
	for(int i : order) {
		const slampp_hip_lm_vertex_range &t = r.p_ranges[i];
		if(t.n_first_vertex != n_covered || t.n_last_vertex > n)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: the vertex ranges do not cover the block columns exactly once");
		const int n_dim = (t.n_vertex_type == SLAMPP_HIP_VERTEX_SE2)? 3 : (t.n_vertex_type == SLAMPP_HIP_VERTEX_SE3)? 6 : 0; // 0: any up to 8
		for(int64_t v = t.n_first_vertex; v < t.n_last_vertex; ++ v) {
			const int64_t d = s.cumsum[v + 1] - s.cumsum[v];
			if((n_dim)? d != n_dim : d > 8)
				return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: a block column does not have the dimension of its vertex range's type");
		}
		n_covered = t.n_last_vertex;
	}
	if(n_covered != n)
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: the vertex ranges do not cover the block columns exactly once");
	if(overlap(r.p_state_dev, r.p_trial_dev, s.n_scalars) || overlap(r.p_state_dev, r.p_dx_dev, s.n_scalars) ||
	   overlap(r.p_trial_dev, r.p_dx_dev, s.n_scalars))
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: state, trial and dx overlap");
	if(!s.Require_Damping_Offsets())
		return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: a block column has no diagonal block");
	return SLAMPP_HIP_OK;
}

// A set whose assembly has a robust specification (slampp_hip_assembly_set_robust): the loop computes
// its weights.  In SLAMPP_HIP_ROBUST_MODE_LOSS the weights are in the set's scaled arrays and the cost is the robust one.
bool is_robust(const slampp_hip_lm_edge_set &t)
{
	return t.p_assembly->b_robust;
}

bool is_robust_loss(const slampp_hip_lm_edge_set &t)
{
	return t.p_assembly->b_robust && t.p_assembly->t_robust.n_mode == SLAMPP_HIP_ROBUST_MODE_LOSS;
}

// the weight array the assembly and the initial damping take for a set: the caller's, or the handle's own (REFERENCE), or none
const double *assembly_weights(const slampp_hip_lm_edge_set &t)
{
	if(!is_robust(t))
		return t.p_weight_dev;
	return (is_robust_loss(t))? 0 : t.p_assembly->d_robust_weight.p();
}

// behind a set's linearize: the weights into the handle's array, and in LOSS the set's Jacobians and errors times sqrt(w)
int robustify(const slampp_hip_lm_edge_set &t)
{
	if(!is_robust(t))
		return SLAMPP_HIP_OK;
	const int n_result = slampp_hip_robust_weights_device_async(t.p_assembly, t.p_sigma_inv_dev, t.p_error_dev, 0);
	if(n_result != SLAMPP_HIP_OK || !is_robust_loss(t))
		return n_result;
	return slampp_hip_robust_scale_device_async(t.p_assembly, 0, t.p_J0_dev, t.p_J1_dev, t.p_error_dev);
}

// errors at p_state_dev (with the Jacobians where b_jacobians is set) and the cost of every set into the parts: chi^2 with
// the caller's weights, of a robust set chi^2 without weights (REFERENCE: SE3_Types.h:323-331) or the robust cost (LOSS), each
// from the unscaled errors -- robustify() comes behind
int errors_and_chi2(const slampp_hip_lm_problem &r, const double *p_state_dev, bool b_jacobians)
{
	for(int i = 0; i < r.n_sets; ++ i) {
		const slampp_hip_lm_edge_set &t = r.p_sets[i];
		int n_result = (b_jacobians)? slampp_hip_linearize_device_async(t.p_assembly, t.n_edge_type, p_state_dev, t.p_measurement_dev,
			t.p_params_dev, t.p_J0_dev, t.p_J1_dev, t.p_error_dev) : slampp_hip_edge_errors_device_async(t.p_assembly, t.n_edge_type,
			p_state_dev, t.p_measurement_dev, t.p_params_dev, t.p_error_dev);
		if(n_result == SLAMPP_HIP_OK) {
			n_result = (is_robust_loss(t))? slampp_hip_robust_chi_squared_device_async(t.p_assembly, t.p_sigma_inv_dev, t.p_error_dev,
				r.p_chi_parts_dev + i) : slampp_hip_chi_squared_device_async(t.p_assembly, t.p_sigma_inv_dev, t.p_error_dev,
				(is_robust(t))? 0 : t.p_weight_dev, r.p_chi_parts_dev + i);
		}
		if(n_result == SLAMPP_HIP_OK && b_jacobians)
			n_result = robustify(t);
		if(n_result != SLAMPP_HIP_OK)
			return n_result;
	}
	return SLAMPP_HIP_OK;
}

void fill_edge_sets(const slampp_hip_lm_problem &r, slampp_hip_edge_set *p_sets)
{
	for(int i = 0; i < r.n_sets; ++ i) {
		const slampp_hip_lm_edge_set &t = r.p_sets[i];
		p_sets[i].p_assembly = t.p_assembly;
		p_sets[i].p_J0_dev = t.p_J0_dev;
		p_sets[i].p_J1_dev = t.p_J1_dev;
		p_sets[i].p_sigma_inv_dev = t.p_sigma_inv_dev;
		p_sets[i].p_error_dev = t.p_error_dev;
		p_sets[i].p_weight_dev = assembly_weights(t);
	}
}

} // anonymous namespace

extern "C" {

int slampp_hip_edge_errors_device_async(slampp_hip_assembly *p_assembly, int n_edge_type, const double *p_state_dev,
	const double *p_measurement_dev, const double *p_params_dev, double *p_error_dev)
{
	if(!p_assembly || !p_assembly->p_solver)
		return SLAMPP_HIP_ERR_INVALID; // (the solver it was created from is gone: nowhere to leave a text)
	slampp_hip_solver *p_solver = p_assembly->p_solver;
	return guarded(p_solver, [&]() -> int {
		if(!p_state_dev || !p_measurement_dev || !p_error_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: null pointer");
		const int n_check = check_edge_set(p_solver, p_assembly, n_edge_type, p_params_dev != 0);
		if(n_check != SLAMPP_HIP_OK)
			return n_check;
		TAsmEdgeView t_edges;
		assembly_edge_view(*p_assembly->p_state, t_edges);
		linearize_enqueue(n_edge_type, t_edges, p_state_dev, p_measurement_dev, p_params_dev, 0, 0, p_error_dev, p_solver->stream);
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_apply_damping_scalar_device_async(slampp_hip_solver *p_solver, double *p_values_dev, const double *p_alpha_dev,
	double f_scale, int64_t n_first_vertex, int64_t n_last_vertex)
{
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		if(!s.b_has_structure)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: set_structure was not called");
		const int64_t n = int64_t(s.cumsum.size()) - 1;
		if(!p_values_dev || !p_alpha_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: null pointer");
		if(n_first_vertex < 0 || n_first_vertex > n_last_vertex || n_last_vertex > n)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: bad vertex range");
		if(!s.Require_Damping_Offsets())
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: a block column has no diagonal block");
		lm_damping_scalar_enqueue(s.d_damp_off.p(), n_first_vertex, n_last_vertex, p_alpha_dev, f_scale, p_values_dev, s.stream);
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_lm_initial_damping_device_async(const slampp_hip_edge_set *p_sets, int n_sets, double f_tau, double *p_alpha_out_dev)
{
	if(!p_sets || n_sets < 1 || !p_sets[0].p_assembly || !p_sets[0].p_assembly->p_solver)
		return SLAMPP_HIP_ERR_INVALID;
	slampp_hip_solver *p_solver = p_sets[0].p_assembly->p_solver;
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		if(n_sets > SLAMPP_HIP_LM_MAX_SETS)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: between 1 and SLAMPP_HIP_LM_MAX_SETS edge sets");
		if(!p_alpha_out_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: null pointer");
		TLmDampingSet p_damping_sets[SLAMPP_HIP_LM_MAX_SETS];
		for(int i = 0; i < n_sets; ++ i) {
			const slampp_hip_edge_set &t = p_sets[i];
			if(!t.p_assembly || t.p_assembly->p_solver != p_solver)
				return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: an edge set's assembly is null or belongs to another solver");
			if(t.p_assembly->b_stale)
				return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: set_structure was called after an assembly was created");
			if(!t.p_J0_dev || !t.p_J1_dev || !t.p_sigma_inv_dev)
				return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: null pointer");
			TAsmEdgeView t_edges;
			assembly_edge_view(*t.p_assembly->p_state, t_edges);
			TLmDampingSet &r_set = p_damping_sets[i];
			r_set.n_edges = t_edges.n_edges;
			r_set.d0 = t_edges.d0; r_set.d1 = t_edges.d1; r_set.rd = t_edges.rd;
			r_set.p_J0 = t.p_J0_dev; r_set.p_J1 = t.p_J1_dev; r_set.p_sigma_inv = t.p_sigma_inv_dev; r_set.p_weight = t.p_weight_dev;
		}
		s.d_lm_reduce.Alloc(size_t(lm_MAX_SETS) * reduce_MAX_PARTIALS);
		lm_initial_damping_enqueue(p_damping_sets, n_sets, f_tau, s.d_lm_reduce.p(), p_alpha_out_dev, s.stream);
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_lm_gain_device_async(slampp_hip_solver *p_solver, const double *p_dx_dev, const double *p_eta_dev, double *p_lm_dev)
{
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		if(s.b_group_active)
			return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, p_s_sharded);
		if(!s.b_has_structure)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: set_structure was not called");
		if(!p_dx_dev || !p_eta_dev || !p_lm_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: null pointer");
		s.d_lm_reduce.Alloc(size_t(lm_MAX_SETS) * reduce_MAX_PARTIALS);
		lm_gain_enqueue(p_dx_dev, p_eta_dev, s.n_scalars, s.d_lm_reduce.p(), p_lm_dev, s.stream);
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_lm_decide_device_async(slampp_hip_solver *p_solver, double *p_lm_dev, const double *p_chi_parts_dev, int n_parts,
	double *p_trace_dev, int64_t n_trace_capacity)
{
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		if(s.b_group_active)
			return fail(p_solver, SLAMPP_HIP_ERR_UNSUPPORTED, p_s_sharded);
		if(!s.b_analyzed || !s.d_flag.p())
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: analyze was not called");
		if(!p_lm_dev || !p_chi_parts_dev || n_trace_capacity < 0)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: null pointer");
		if(n_parts < 1 || n_parts > SLAMPP_HIP_LM_MAX_SETS)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: between 1 and SLAMPP_HIP_LM_MAX_SETS edge sets");
		lm_decide_enqueue(p_lm_dev, p_chi_parts_dev, n_parts, s.d_flag.p(), p_trace_dev, n_trace_capacity, s.stream);
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_lm_commit_device_async(slampp_hip_solver *p_solver, const double *p_lm_dev, double *p_state_dev,
	const double *p_trial_dev)
{
	return guarded(p_solver, [&]() -> int {
		slampp_hip_solver &s = *p_solver;
		if(!s.b_has_structure)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: set_structure was not called");
		if(!p_lm_dev || !p_state_dev || !p_trial_dev)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: null pointer");
		if(overlap(p_state_dev, p_trial_dev, s.n_scalars))
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: state, trial and dx overlap");
		lm_commit_enqueue(p_lm_dev, p_state_dev, p_trial_dev, s.n_scalars, s.stream);
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_lm_begin_device_async(const slampp_hip_lm_problem *p_problem, double f_alpha, double f_tau, double f_min_dx_norm,
	int n_max_iterations, int n_extra_on_reject)
{
	if(!p_problem || !p_problem->p_solver)
		return SLAMPP_HIP_ERR_INVALID;
	const slampp_hip_lm_problem &r = *p_problem;
	slampp_hip_solver *p_solver = r.p_solver;
	int n_result = guarded(p_solver, [&]() -> int { return check_problem(r); });
	if(n_result != SLAMPP_HIP_OK)
		return n_result;
	const bool b_initial_damping = f_tau > 0;
	if((n_result = errors_and_chi2(r, r.p_state_dev, b_initial_damping)) != SLAMPP_HIP_OK)
		return n_result;
	if(b_initial_damping) { // (into the block itself: lm_begin_kernel reads it before it writes)
		slampp_hip_edge_set p_sets[SLAMPP_HIP_LM_MAX_SETS];
		fill_edge_sets(r, p_sets);
		if((n_result = slampp_hip_lm_initial_damping_device_async(p_sets, r.n_sets, f_tau, r.p_lm_dev + SLAMPP_HIP_LM_ALPHA)) != SLAMPP_HIP_OK)
			return n_result;
	}
	return guarded(p_solver, [&]() -> int {
		lm_begin_enqueue(r.p_lm_dev, (b_initial_damping)? r.p_lm_dev + SLAMPP_HIP_LM_ALPHA : 0, f_alpha, r.p_chi_parts_dev, r.n_sets,
			f_min_dx_norm, n_max_iterations, n_extra_on_reject, p_solver->stream);
		return SLAMPP_HIP_OK;
	});
}

int slampp_hip_lm_iterate_device_async(const slampp_hip_lm_problem *p_problem, int n_rounds)
{
	if(!p_problem || !p_problem->p_solver)
		return SLAMPP_HIP_ERR_INVALID;
	const slampp_hip_lm_problem &r = *p_problem;
	slampp_hip_solver *p_solver = r.p_solver;
	int n_result = guarded(p_solver, [&]() -> int {
		if(n_rounds <= 0)
			return fail(p_solver, SLAMPP_HIP_ERR_INVALID, "lm: n_rounds is not positive");
		return check_problem(r);
	});
	if(n_result != SLAMPP_HIP_OK)
		return n_result;
	slampp_hip_edge_set p_sets[SLAMPP_HIP_LM_MAX_SETS];
	fill_edge_sets(r, p_sets);
	const int64_t n_bcols = int64_t(p_solver->cumsum.size()) - 1;
	const size_t n_vector_bytes = size_t(p_solver->n_scalars) * sizeof(double);
#define LM_STEP(call) do { if((n_result = (call)) != SLAMPP_HIP_OK) return n_result; } while(0)
	for(int n_round = 0; n_round < n_rounds; ++ n_round) {
		for(int i = 0; i < r.n_sets; ++ i) {
			const slampp_hip_lm_edge_set &t = r.p_sets[i];
			LM_STEP(slampp_hip_linearize_device_async(t.p_assembly, t.n_edge_type, r.p_state_dev, t.p_measurement_dev, t.p_params_dev,
				t.p_J0_dev, t.p_J1_dev, t.p_error_dev));
			LM_STEP(robustify(t));
		}
		LM_STEP(slampp_hip_assemble_sets_device_async(p_sets, r.n_sets, r.n_unary_vertex, r.p_unary_factor, r.p_unary_error,
			r.p_values_dev, r.p_eta_dev, 0));
		LM_STEP(guarded(p_solver, [&]() -> int { // dx = eta: the solve overwrites its right-hand side, the gain ratio needs both
			SLAMPP_HIP_CHECK(hipMemcpyAsync(r.p_dx_dev, r.p_eta_dev, n_vector_bytes, hipMemcpyDeviceToDevice, p_solver->stream));
			return SLAMPP_HIP_OK;
		}));
		LM_STEP(slampp_hip_apply_damping_scalar_device_async(p_solver, r.p_values_dev, r.p_lm_dev + SLAMPP_HIP_LM_ALPHA, 1.0, 0, n_bcols));
		LM_STEP(slampp_hip_factor_solve_device_async(p_solver, r.p_values_dev, r.p_dx_dev));
		LM_STEP(slampp_hip_lm_gain_device_async(p_solver, r.p_dx_dev, r.p_eta_dev, r.p_lm_dev));
		for(int i = 0; i < r.n_ranges; ++ i) {
			const slampp_hip_lm_vertex_range &t = r.p_ranges[i];
			LM_STEP(slampp_hip_state_plus_device_async(p_solver, t.n_vertex_type, t.n_first_vertex, t.n_last_vertex, r.p_state_dev,
				r.p_dx_dev, 1.0, r.p_trial_dev));
		}
		LM_STEP(errors_and_chi2(r, r.p_trial_dev, false));
		LM_STEP(slampp_hip_lm_decide_device_async(p_solver, r.p_lm_dev, r.p_chi_parts_dev, r.n_sets, r.p_trace_dev, r.n_trace_capacity));
		LM_STEP(slampp_hip_lm_commit_device_async(p_solver, r.p_lm_dev, r.p_state_dev, r.p_trial_dev));
	}
#undef LM_STEP
	return SLAMPP_HIP_OK;
}

} // extern "C"
