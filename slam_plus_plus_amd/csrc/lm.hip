// lm.hip -- the Levenberg-Marquardt loop's accept / reject and damping rule on the device (lm.h): the initial damping, the
// damping from a scalar in device memory, the two dot products of the gain ratio in one pass, the decision on the block of
// scalars, and the commit of an accepted trial state.  Shaped like linearize.hip: wave64, a lane per item unless stated,
// plain fp64, no atomics, fixed summation orders -- the same call twice gives the same bits.  Every value is written by an
// ordinary vector store from plain C++.
#include "lm.h"
#include "multiply.h"

#include <algorithm>

namespace slampp {

enum { A = SLAMPP_HIP_LM_ALPHA, NU = SLAMPP_HIP_LM_NU, LAST = SLAMPP_HIP_LM_LAST_ERROR, ERR = SLAMPP_HIP_LM_ERROR,
	DXDX = SLAMPP_HIP_LM_DX_DX, DXETA = SLAMPP_HIP_LM_DX_ETA, RHO = SLAMPP_HIP_LM_RHO, ACC = SLAMPP_HIP_LM_ACCEPTED,
	STATUS = SLAMPP_HIP_LM_STATUS, ROUNDS = SLAMPP_HIP_LM_N_ROUNDS, N_ACC = SLAMPP_HIP_LM_N_ACCEPTED,
	N_REJ = SLAMPP_HIP_LM_N_REJECTED, LEFT = SLAMPP_HIP_LM_ROUNDS_LEFT, EXTRA = SLAMPP_HIP_LM_EXTRA_LEFT,
	MIN_DX = SLAMPP_HIP_LM_MIN_DX_NORM, RECORDS = SLAMPP_HIP_LM_N_RECORDS };
static_assert(lm_MAX_SETS == SLAMPP_HIP_LM_MAX_SETS && lm_TRACE_RECORD == SLAMPP_HIP_LM_TRACE_RECORD, "include/slampp_hip.h and lm.h disagree");

// ---- workgroup reductions of 256 threads (the result in thread 0); s_red: 4 doubles of LDS per call site ----

__device__ __forceinline__ double lm_workgroup_sum(double f_acc, double *s_red) // (the tree of reduce_workgroup, multiply.hip)
{
	#pragma unroll
	for(int m = 1; m < 64; m <<= 1)
		f_acc += __shfl_xor(f_acc, m);
	if(threadIdx.x % 64 == 0)
		s_red[threadIdx.x / 64] = f_acc;
	__syncthreads();
	return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

__device__ __forceinline__ double lm_max(double a, double b) // (std::max(a, b): b enters only where it is greater; a NaN never does)
{
	return (b > a)? b : a;
}

__device__ __forceinline__ double lm_workgroup_max(double f_acc, double *s_red)
{
	#pragma unroll
	for(int m = 1; m < 64; m <<= 1)
		f_acc = lm_max(f_acc, __shfl_xor(f_acc, m));
	if(threadIdx.x % 64 == 0)
		s_red[threadIdx.x / 64] = f_acc;
	__syncthreads();
	return lm_max(lm_max(s_red[0], s_red[1]), lm_max(s_red[2], s_red[3]));
}

// ---- the initial damping ----

// the largest diagonal entry of J^T Omega J, J column-major rd x d: column j gives sum_c (sum_r J_rj Omega_rc) J_cj
__device__ __forceinline__ double lm_max_hessian_diag(const double *__restrict__ p_J, const double *__restrict__ p_omega, int rd, int d,
	double f_weight, double f_max)
{
	for(int j = 0; j < d; ++ j) {
		const double *p_col = p_J + j * rd;
		double f_diag = 0;
		for(int c = 0; c < rd; ++ c) {
			double f_dot = 0;
			for(int r = 0; r < rd; ++ r)
				f_dot += p_col[r] * p_omega[r + c * rd];
			f_diag += f_dot * p_col[c];
		}
		f_max = lm_max(f_max, f_weight * f_diag);
	}
	return f_max;
}

// a lane per edge (grid-stride); the workgroup's maximum to p_partial[blockIdx.x]
__global__ void __launch_bounds__(256)
lm_damping_first_kernel(TLmDampingSet t_set, double *p_partial)
{
	__shared__ double s_red[4];
	const int64_t n_stride = int64_t(gridDim.x) * 256;
	const int rd = t_set.rd, d0 = t_set.d0, d1 = t_set.d1;
	double f_max = 0;
	for(int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < t_set.n_edges; e += n_stride) {
		const double *p_omega = t_set.p_sigma_inv + e * rd * rd;
		const double f_weight = (t_set.p_weight)? t_set.p_weight[e] : 1.0;
		f_max = lm_max_hessian_diag(t_set.p_J0 + e * rd * d0, p_omega, rd, d0, f_weight, f_max);
		f_max = lm_max_hessian_diag(t_set.p_J1 + e * rd * d1, p_omega, rd, d1, f_weight, f_max);
	}
	f_max = lm_workgroup_max(f_max, s_red);
	if(threadIdx.x == 0)
		p_partial[blockIdx.x] = f_max;
}

struct TLmPartialList {
	int n_sets;
	int p_count[lm_MAX_SETS]; // the partial maxima of set i: p_count[i] doubles at p_partials + i * reduce_MAX_PARTIALS
};

__global__ void __launch_bounds__(256)
lm_damping_second_kernel(const double *__restrict__ p_partials, TLmPartialList t_list, double f_tau, double *p_out)
{
	__shared__ double s_red[4];
	double f_max = 0;
	for(int s = 0; s < t_list.n_sets; ++ s) {
		for(int i = threadIdx.x; i < t_list.p_count[s]; i += 256)
			f_max = lm_max(f_max, p_partials[s * reduce_MAX_PARTIALS + i]);
	}
	f_max = lm_workgroup_max(f_max, s_red);
	if(threadIdx.x == 0)
		*p_out = f_max * f_tau;
}

void lm_initial_damping_enqueue(const TLmDampingSet *p_sets, int n_sets, double f_tau, double *p_partials, double *p_alpha_out,
	hipStream_t stream)
{
	if(n_sets < 1 || n_sets > lm_MAX_SETS)
		throw std::invalid_argument("lm: between 1 and SLAMPP_HIP_LM_MAX_SETS edge sets");
	TLmPartialList t_list;
	t_list.n_sets = n_sets;
	for(int i = 0; i < lm_MAX_SETS; ++ i)
		t_list.p_count[i] = 0;
	for(int i = 0; i < n_sets; ++ i) {
		const TLmDampingSet &t = p_sets[i];
		if(t.rd < 1 || t.rd > lm_MAX_DIM || t.d0 < 1 || t.d0 > lm_MAX_DIM || t.d1 < 1 || t.d1 > lm_MAX_DIM)
			throw std::domain_error("lm: the initial damping takes edge sets with rd, d0, d1 <= 8");
		const int n_groups = int(std::min<int64_t>(reduce_MAX_PARTIALS, std::max<int64_t>(1, (t.n_edges + 255) / 256))); // (of n_edges alone)
		t_list.p_count[i] = n_groups;
		hipLaunchKernelGGL(lm_damping_first_kernel, dim3(n_groups), dim3(256), 0, stream, t, p_partials + size_t(i) * reduce_MAX_PARTIALS);
	}
	hipLaunchKernelGGL(lm_damping_second_kernel, dim3(1), dim3(256), 0, stream, p_partials, t_list, f_tau, p_alpha_out);
	SLAMPP_HIP_CHECK(hipGetLastError());
}

// ---- damping from a device scalar (damping_kernel of assembly.hip with alpha fetched by every lane) ----

__global__ void __launch_bounds__(256)
lm_damping_scalar_kernel(const int64_t *__restrict__ p_off_dim, int64_t n_first, int64_t n_last, const double *__restrict__ p_alpha,
	double f_scale, double *p_values)
{
	const int64_t v = n_first + int64_t(blockIdx.x) * 256 + threadIdx.x;
	if(v >= n_last)
		return;
	const double f_alpha = *p_alpha * f_scale;
	const int64_t n_off = p_off_dim[2 * v], d = p_off_dim[2 * v + 1];
	for(int64_t r = 0; r < d; ++ r)
		p_values[n_off + r * (d + 1)] += f_alpha;
}

void lm_damping_scalar_enqueue(const int64_t *p_off_dim_dev, int64_t n_first, int64_t n_last, const double *p_alpha, double f_scale,
	double *p_values_dev, hipStream_t stream)
{
	if(n_last <= n_first)
		return;
	const int64_t n_grid = (n_last - n_first + 255) / 256;
	if(n_grid > 0x7fffffff)
		throw std::domain_error("lm: too many block columns");
	hipLaunchKernelGGL(lm_damping_scalar_kernel, dim3(unsigned(n_grid)), dim3(256), 0, stream, p_off_dim_dev, n_first, n_last, p_alpha,
		f_scale, p_values_dev);
	SLAMPP_HIP_CHECK(hipGetLastError());
}

// ---- the gain ratio's two dot products: reduce_first_kernel / reduce_second_kernel (multiply.hip) on two sums at once ----

__global__ void __launch_bounds__(256)
lm_gain_first_kernel(const double *__restrict__ p_dx, const double *__restrict__ p_eta, int64_t n, double *p_partial)
{
	__shared__ double s_red[2][4];
	const int64_t n_stride = int64_t(gridDim.x) * 256;
	double f_dd = 0, f_de = 0;
	for(int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += n_stride) {
		const double d = p_dx[i];
		f_dd += d * d;
		f_de += d * p_eta[i];
	}
	f_dd = lm_workgroup_sum(f_dd, s_red[0]);
	f_de = lm_workgroup_sum(f_de, s_red[1]);
	if(threadIdx.x == 0) {
		p_partial[blockIdx.x] = f_dd;
		p_partial[reduce_MAX_PARTIALS + blockIdx.x] = f_de;
	}
}

__global__ void __launch_bounds__(256)
lm_gain_second_kernel(const double *__restrict__ p_partial, int n_partials, double *p_lm)
{
	__shared__ double s_red[2][4];
	double f_dd = 0, f_de = 0;
	for(int i = threadIdx.x; i < n_partials; i += 256) {
		f_dd += p_partial[i];
		f_de += p_partial[reduce_MAX_PARTIALS + i];
	}
	f_dd = lm_workgroup_sum(f_dd, s_red[0]);
	f_de = lm_workgroup_sum(f_de, s_red[1]);
	if(threadIdx.x == 0 && p_lm[STATUS] == 0) {
		p_lm[DXDX] = f_dd;
		p_lm[DXETA] = f_de;
	}
}

void lm_gain_enqueue(const double *p_dx, const double *p_eta, int64_t n, double *p_partials, double *p_lm, hipStream_t stream)
{
	const int n_groups = int(std::min<int64_t>(reduce_MAX_PARTIALS, std::max<int64_t>(1, (n + 1023) / 1024))); // (of n alone, as dot_enqueue)
	hipLaunchKernelGGL(lm_gain_first_kernel, dim3(n_groups), dim3(256), 0, stream, p_dx, p_eta, n, p_partials);
	hipLaunchKernelGGL(lm_gain_second_kernel, dim3(1), dim3(256), 0, stream, p_partials, n_groups, p_lm);
	SLAMPP_HIP_CHECK(hipGetLastError());
}

// ---- the decision: NonlinearSolver_Lambda_LM.h:972 (the factorization failed), :1054 (the step is small), :207-222
// (Aftermath), :1103-1106 (the extra iterations), :919 (the loop's bound), by one lane ----

__global__ void __launch_bounds__(64)
lm_decide_kernel(double *p_lm, const double *__restrict__ p_chi_parts, int n_parts, const int *__restrict__ p_flag, double *p_trace,
	int64_t n_trace)
{
	#pragma clang fp contract(off) // (the rule as the host compiles it: alpha * dx^T dx + dx^T eta and 1 - t^3 round every product)
	if(threadIdx.x != 0 || blockIdx.x != 0)
		return;
	if(p_lm[STATUS] != 0) {
		p_lm[ACC] = 0;
		return;
	}
	double f_error = 0;
	for(int i = 0; i < n_parts; ++ i)
		f_error += p_chi_parts[i];
	const double f_alpha_used = p_lm[A], f_dx_dx = p_lm[DXDX], f_dx_norm = sqrt(f_dx_dx);
	double f_alpha = f_alpha_used, f_nu = p_lm[NU], f_last = p_lm[LAST], f_rho = 0, f_accepted = 0, f_status = 0;
	if(*p_flag != 0)
		f_status = SLAMPP_HIP_LM_STATUS_NOT_POSDEF;
	else if(f_dx_norm <= p_lm[MIN_DX])
		f_status = SLAMPP_HIP_LM_STATUS_CONVERGED;
	else {
		f_rho = (f_last - f_error) / (f_alpha * f_dx_dx + p_lm[DXETA]);
		if(f_rho > 0) { // (the only test: a NaN rejects)
			const double t = 2 * f_rho - 1, f_cap = 1.0 - t * t * t; // (t * t * t for pow(t, 3))
			f_alpha *= (f_cap > 1 / 3.0)? f_cap : 1 / 3.0; // (std::max(1 / 3.0, cap))
			f_nu = 2;
			f_last = f_error;
			f_accepted = 1;
			p_lm[N_ACC] += 1;
		} else {
			f_alpha *= f_nu;
			f_nu *= 2;
			p_lm[N_REJ] += 1;
			if(p_lm[EXTRA] > 0) {
				p_lm[EXTRA] -= 1;
				p_lm[LEFT] += 1;
			}
		}
		const double f_left = p_lm[LEFT] - 1;
		p_lm[LEFT] = f_left;
		if(f_left <= 0)
			f_status = SLAMPP_HIP_LM_STATUS_BUDGET;
	}
	p_lm[A] = f_alpha;
	p_lm[NU] = f_nu;
	p_lm[LAST] = f_last;
	p_lm[ERR] = f_error;
	p_lm[RHO] = f_rho;
	p_lm[ACC] = f_accepted;
	p_lm[STATUS] = f_status;
	p_lm[ROUNDS] += 1;
	const double f_record = p_lm[RECORDS];
	p_lm[RECORDS] = f_record + 1;
	if(p_trace && f_record < double(n_trace)) {
		double *p_record = p_trace + int64_t(f_record) * lm_TRACE_RECORD;
		p_record[SLAMPP_HIP_LM_TRACE_ALPHA] = f_alpha_used;
		p_record[SLAMPP_HIP_LM_TRACE_ERROR] = f_error;
		p_record[SLAMPP_HIP_LM_TRACE_RHO] = f_rho;
		p_record[SLAMPP_HIP_LM_TRACE_DX_NORM] = f_dx_norm;
		p_record[SLAMPP_HIP_LM_TRACE_ACCEPTED] = f_accepted;
		p_record[SLAMPP_HIP_LM_TRACE_STATUS] = f_status;
		p_record[SLAMPP_HIP_LM_TRACE_LAST_ERROR] = f_last;
		p_record[SLAMPP_HIP_LM_TRACE_NU] = f_nu;
	}
}

void lm_decide_enqueue(double *p_lm, const double *p_chi_parts, int n_parts, const int *p_flag, double *p_trace, int64_t n_trace,
	hipStream_t stream)
{
	hipLaunchKernelGGL(lm_decide_kernel, dim3(1), dim3(64), 0, stream, p_lm, p_chi_parts, n_parts, p_flag, p_trace, n_trace);
	SLAMPP_HIP_CHECK(hipGetLastError());
}

// ---- the commit: a lane per 16 bytes where state and trial share their alignment modulo 16 (a leading and a trailing
// double go with lane 0), a lane per two doubles otherwise.  Every lane reads ACCEPTED: uniform, nothing to synchronize ----

__global__ void __launch_bounds__(256)
lm_commit_kernel(const double *__restrict__ p_lm, double *__restrict__ p_state, const double *__restrict__ p_trial, int64_t n)
{
	if(p_lm[ACC] == 0)
		return;
	const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
	if(((reinterpret_cast<uintptr_t>(p_state) ^ reinterpret_cast<uintptr_t>(p_trial)) & 15) == 0) {
		const int64_t n_head = ((reinterpret_cast<uintptr_t>(p_state) & 15) && n > 0)? 1 : 0, n_pairs = (n - n_head) / 2;
		if(i < n_pairs)
			reinterpret_cast<double2*>(p_state + n_head)[i] = reinterpret_cast<const double2*>(p_trial + n_head)[i];
		if(i == 0) {
			if(n_head)
				p_state[0] = p_trial[0];
			if((n - n_head) & 1)
				p_state[n - 1] = p_trial[n - 1];
		}
	} else {
		if(2 * i < n)
			p_state[2 * i] = p_trial[2 * i];
		if(2 * i + 1 < n)
			p_state[2 * i + 1] = p_trial[2 * i + 1];
	}
}

void lm_commit_enqueue(const double *p_lm, double *p_state, const double *p_trial, int64_t n, hipStream_t stream)
{
	if(n < 1)
		return;
	const int64_t n_grid = ((n + 1) / 2 + 255) / 256; // (a lane per pair; n = 1 with a head: lane 0)
	if(n_grid > 0x7fffffff)
		throw std::domain_error("lm: too many scalars");
	hipLaunchKernelGGL(lm_commit_kernel, dim3(unsigned(n_grid)), dim3(256), 0, stream, p_lm, p_state, p_trial, n);
	SLAMPP_HIP_CHECK(hipGetLastError());
}

// ---- the scalars of a new loop ----

__global__ void __launch_bounds__(64)
lm_begin_kernel(double *p_lm, const double *p_alpha_dev, double f_alpha, const double *__restrict__ p_chi_parts, int n_parts,
	double f_min_dx_norm, int n_max_iterations, int n_extra_on_reject)
{
	if(threadIdx.x != 0 || blockIdx.x != 0)
		return;
	const double f_alpha_start = (p_alpha_dev)? *p_alpha_dev : f_alpha; // (read before the block is written: it may lie inside)
	double f_error = 0;
	for(int i = 0; i < n_parts; ++ i)
		f_error += p_chi_parts[i];
	for(int i = 0; i < SLAMPP_HIP_LM_SCALARS; ++ i)
		p_lm[i] = 0;
	p_lm[A] = f_alpha_start;
	p_lm[NU] = 2;
	p_lm[LAST] = f_error;
	p_lm[MIN_DX] = f_min_dx_norm;
	p_lm[LEFT] = (n_max_iterations > 0)? n_max_iterations : 0;
	p_lm[EXTRA] = (n_extra_on_reject > 0)? n_extra_on_reject : 0;
	p_lm[STATUS] = (n_max_iterations > 0)? SLAMPP_HIP_LM_STATUS_RUNNING : SLAMPP_HIP_LM_STATUS_BUDGET;
}

void lm_begin_enqueue(double *p_lm, const double *p_alpha_dev, double f_alpha, const double *p_chi_parts, int n_parts,
	double f_min_dx_norm, int n_max_iterations, int n_extra_on_reject, hipStream_t stream)
{
	hipLaunchKernelGGL(lm_begin_kernel, dim3(1), dim3(64), 0, stream, p_lm, p_alpha_dev, f_alpha, p_chi_parts, n_parts, f_min_dx_norm,
		n_max_iterations, n_extra_on_reject);
	SLAMPP_HIP_CHECK(hipGetLastError());
}

} // namespace slampp
