// robust.hip -- robust kernels on the device (robust.h): every edge's weight w(s), the scaling of an edge set by sqrt(w) and the
// robust cost.  Shaped like linearize.hip, walked the other way: the records of the 64 edges of a tile are one run in memory
// (Omega: 64 rd^2 doubles, err: 64 rd), which the workgroup loads as whole lines into an LDS tile of one row per edge; a lane
// then reads its own row.  A lane loading its own record from memory would touch 64 lines per instruction (what chi2_first_kernel
// does: DESIGN.md section 4.9 measured it at 5 copies).  Plain fp64, no atomics, fixed summation orders -- the same call twice
// gives the same bits.  Every value is written by an ordinary vector store from plain C++.
#include "robust.h"
#include "multiply.h"

#include <algorithm>

namespace slampp {

// ---- the loss functions: w(s) to the expressions of RobustLoss.h, in their order and without contraction; rho with
// rho' = s w(s) and rho(0) = 0 ----

__device__ __forceinline__ double robust_weight(int n_kernel, double a, double s)
{
	#pragma clang fp contract(off)
	switch(n_kernel) {
	case SLAMPP_HIP_ROBUST_HUBER:
		return (s <= a)? 1 : a / s; // :103
	case SLAMPP_HIP_ROBUST_CAUCHY:
		return a * a / (a * a + s * s); // :153
	case SLAMPP_HIP_ROBUST_TUKEY:
		return (s <= a)? (1 - (s * s) / (a * a)) * (1 - (s * s) / (a * a)) : 0; // :206
	default:
		return exp(-s * s / (a * a)); // :433 (SLAMPP_HIP_ROBUST_WELSCH)
	}
}

__device__ __forceinline__ double robust_rho(int n_kernel, double a, double s)
{
	#pragma clang fp contract(off)
	switch(n_kernel) {
	case SLAMPP_HIP_ROBUST_HUBER:
		return (s <= a)? s * s / 2 : a * (s - a / 2);
	case SLAMPP_HIP_ROBUST_CAUCHY:
		return (a * a / 2) * log1p(s * s / (a * a));
	case SLAMPP_HIP_ROBUST_TUKEY:
		{
			if(!(s <= a))
				return a * a / 6;
			const double t = 1 - (s * s) / (a * a);
			return (a * a / 6) * (1 - t * t * t);
		}
	default:
		return (a * a / 2) * -expm1(-s * s / (a * a));
	}
}

// ---- a run of n_here records of N doubles, from memory into a tile of one row of N | 1 doubles per record.  Consecutive lanes
// load consecutive doubles: 16 bytes a lane where the run begins on a 16-byte boundary (a tile of 64 records begins 64 N 8
// bytes from the array's base: the alignment is the array's), 8 otherwise.  The lane that later walks down a tile column has an
// odd stride in doubles and spreads over the banks (the tile of store_through_tile, linearize.hip, walked the other way).
// T: the threads of the workgroup.  The caller synchronizes. ----

template <int N, int T>
__device__ __forceinline__ void load_through_tile(double *p_tile, const double *__restrict__ p_src, int n_here)
{
	enum { STRIDE = N | 1 };
	const int n = n_here * N;
	if((reinterpret_cast<uintptr_t>(p_src) & 15) == 0) {
		for(int i = 2 * int(threadIdx.x); i + 1 < n; i += 2 * T) {
			const double2 v = *reinterpret_cast<const double2*>(p_src + i);
			p_tile[(i / N) * STRIDE + i % N] = v.x;
			p_tile[((i + 1) / N) * STRIDE + (i + 1) % N] = v.y;
		}
		if((n & 1) && threadIdx.x == 0)
			p_tile[((n - 1) / N) * STRIDE + (n - 1) % N] = p_src[n - 1];
	} else {
		for(int i = threadIdx.x; i < n; i += T)
			p_tile[(i / N) * STRIDE + i % N] = p_src[i];
	}
}

// err^T Omega err of a tile row, Omega column-major and summed column by column: the order of chi2_first_kernel
template <int RD>
__device__ __forceinline__ double robust_quadratic_form(const double *p_omega_row, const double (&err)[RD])
{
	double f_term = 0;
	#pragma unroll
	for(int c = 0; c < RD; ++ c) {
		double f_col = 0;
		#pragma unroll
		for(int r = 0; r < RD; ++ r)
			f_col += err[r] * p_omega_row[r + c * RD];
		f_term += f_col * err[c];
	}
	return f_term;
}

struct TRobustParams { // a checked slampp_hip_robust as the kernels take it
	int n_kernel, n_basis;
	double f_scale, f_param;
};

// ---- the weights: a lane per edge, robust_TILE_EDGES edges per workgroup; b_omega = false (the basis is the error's norm):
// Omega is not read and the tile is the errors' alone.  One tile serves both arrays: the errors go to registers first ----

template <int RD, bool b_omega>
__global__ void __launch_bounds__(robust_TILE_EDGES)
robust_weights_kernel(TRobustParams t, int64_t n_edges, const double *__restrict__ p_sigma_inv, const double *__restrict__ p_error,
	double *__restrict__ p_weight)
{
	enum { N = (b_omega)? RD * RD : RD };
	__shared__ double p_tile[robust_TILE_EDGES * (N | 1)];
	const int64_t n_first = int64_t(blockIdx.x) * robust_TILE_EDGES, e = n_first + threadIdx.x;
	const int n_here = (n_edges - n_first < robust_TILE_EDGES)? int(n_edges - n_first) : int(robust_TILE_EDGES);
	const bool b_mine = e < n_edges;
	load_through_tile<RD, robust_TILE_EDGES>(p_tile, p_error + n_first * RD, n_here);
	__syncthreads();
	double err[RD];
	#pragma unroll
	for(int k = 0; k < RD; ++ k)
		err[k] = (b_mine)? p_tile[threadIdx.x * (RD | 1) + k] : 0.0;
	double f_square; // |err|^2, or err^T Omega err
	if(b_omega) {
		__syncthreads(); // (the tile is used again)
		load_through_tile<RD * RD, robust_TILE_EDGES>(p_tile, p_sigma_inv + n_first * RD * RD, n_here);
		__syncthreads();
		f_square = (b_mine)? robust_quadratic_form<RD>(p_tile + threadIdx.x * (RD * RD | 1), err) : 0.0;
	} else {
		f_square = 0;
		#pragma unroll
		for(int k = 0; k < RD; ++ k)
			f_square += err[k] * err[k];
	}
	if(b_mine) {
		const double s = ((t.n_basis == SLAMPP_HIP_ROBUST_BASIS_CHI2)? f_square : sqrt(f_square)) / t.f_scale;
		p_weight[e] = robust_weight(t.n_kernel, t.f_param, s); // (consecutive lanes, consecutive doubles)
	}
}

void robust_weights_enqueue(const slampp_hip_robust &r_spec, int64_t n_edges, int rd, const double *p_sigma_inv,
	const double *p_error, double *p_weight, hipStream_t stream)
{
	const int64_t n_grid = (n_edges + robust_TILE_EDGES - 1) / robust_TILE_EDGES;
	if(n_grid < 1)
		return;
	if(n_grid > 0x7fffffff)
		throw std::domain_error("robust: too many edges");
	const TRobustParams t = { r_spec.n_kernel, r_spec.n_basis, r_spec.f_scale, r_spec.f_param };
	const bool b_omega = r_spec.n_basis != SLAMPP_HIP_ROBUST_BASIS_ERROR_NORM;
#define LAUNCH_WEIGHTS(RD) case RD: if(b_omega) hipLaunchKernelGGL((robust_weights_kernel<RD, true>), dim3(unsigned(n_grid)), \
		dim3(robust_TILE_EDGES), 0, stream, t, n_edges, p_sigma_inv, p_error, p_weight); \
	else hipLaunchKernelGGL((robust_weights_kernel<RD, false>), dim3(unsigned(n_grid)), dim3(robust_TILE_EDGES), 0, stream, t, \
		n_edges, p_sigma_inv, p_error, p_weight); break
	switch(rd) {
	LAUNCH_WEIGHTS(1); LAUNCH_WEIGHTS(2); LAUNCH_WEIGHTS(3); LAUNCH_WEIGHTS(4);
	LAUNCH_WEIGHTS(5); LAUNCH_WEIGHTS(6); LAUNCH_WEIGHTS(7); LAUNCH_WEIGHTS(8);
	default: throw std::domain_error("robust: edge sets with rd <= 8");
	}
#undef LAUNCH_WEIGHTS
	SLAMPP_HIP_CHECK(hipGetLastError());
}

// ---- the scaling: flat over the pairs of consecutive doubles of J0, then of J1, then of err; a lane takes a pair (16 bytes
// where the array begins on a 16-byte boundary) and looks the weight of each element's edge up -- one line of the weights for
// a whole wave.  An odd array's last element is a pair of one. ----

__device__ __forceinline__ void robust_scale_pair(double *p_array, uint32_t n, uint32_t n_record, const double *__restrict__ p_weight,
	uint32_t n_pair)
{
	const uint32_t i = 2 * n_pair;
	if(i + 1 < n) {
		const double f_w0 = sqrt(p_weight[i / n_record]), f_w1 = sqrt(p_weight[(i + 1) / n_record]);
		if((reinterpret_cast<uintptr_t>(p_array) & 15) == 0) {
			double2 v = reinterpret_cast<double2*>(p_array)[n_pair];
			v.x *= f_w0;
			v.y *= f_w1;
			reinterpret_cast<double2*>(p_array)[n_pair] = v;
		} else {
			p_array[i] *= f_w0;
			p_array[i + 1] *= f_w1;
		}
	} else if(i < n)
		p_array[i] *= sqrt(p_weight[i / n_record]);
}

__global__ void __launch_bounds__(256)
robust_scale_kernel(uint32_t n_J0, uint32_t n_J1, uint32_t n_err, uint32_t n_record_J0, uint32_t n_record_J1, uint32_t n_record_err,
	const double *__restrict__ p_weight, double *p_J0, double *p_J1, double *p_error)
{
	const uint32_t n_pairs_J0 = (n_J0 + 1) / 2, n_pairs_J1 = (n_J1 + 1) / 2, n_pairs_err = (n_err + 1) / 2;
	uint32_t n_pair = blockIdx.x * 256u + threadIdx.x;
	if(n_pair < n_pairs_J0)
		robust_scale_pair(p_J0, n_J0, n_record_J0, p_weight, n_pair);
	else if((n_pair -= n_pairs_J0) < n_pairs_J1)
		robust_scale_pair(p_J1, n_J1, n_record_J1, p_weight, n_pair);
	else if((n_pair -= n_pairs_J1) < n_pairs_err)
		robust_scale_pair(p_error, n_err, n_record_err, p_weight, n_pair);
}

void robust_scale_enqueue(int64_t n_edges, int rd, int d0, int d1, const double *p_weight, double *p_J0, double *p_J1,
	double *p_error, hipStream_t stream)
{
	if(n_edges < 1)
		return;
	if(rd < 1 || rd > robust_MAX_DIM || d0 < 1 || d0 > robust_MAX_DIM || d1 < 1 || d1 > robust_MAX_DIM)
		throw std::domain_error("robust: edge sets with rd, d0, d1 <= 8");
	const int64_t n_J0 = n_edges * rd * d0, n_J1 = n_edges * rd * d1, n_err = n_edges * rd;
	const int64_t n_pairs = (n_J0 + 1) / 2 + (n_J1 + 1) / 2 + (n_err + 1) / 2;
	if(n_J0 + n_J1 + n_err > 0x7fffffff) // (the kernel's indices are 32-bit: its divisions are)
		throw std::domain_error("robust: too many edges");
	hipLaunchKernelGGL(robust_scale_kernel, dim3(unsigned((n_pairs + 255) / 256)), dim3(256), 0, stream, uint32_t(n_J0), uint32_t(n_J1),
		uint32_t(n_err), uint32_t(rd * d0), uint32_t(rd * d1), uint32_t(rd), p_weight, p_J0, p_J1, p_error);
	SLAMPP_HIP_CHECK(hipGetLastError());
}

// ---- the robust cost: the two passes of chi2_enqueue (linearize.hip) -- thread t of workgroup g takes the edges
// 256 g + t + k 256 gridDim.x in ascending order, the workgroup adds its threads' sums in the same tree -- with
// 2 scale^2 rho(s) in the place of the term.  The 256 edges of a step are four tiles, staged one after the other by the whole
// workgroup; wave j computes on tile j. ----

__device__ __forceinline__ double robust_workgroup_sum(double f_acc) // 256 threads; the result in thread 0 (chi2_workgroup_sum)
{
	__shared__ double s_red[4];
	#pragma unroll
	for(int m = 1; m < 64; m <<= 1)
		f_acc += __shfl_xor(f_acc, m);
	if(threadIdx.x % 64 == 0)
		s_red[threadIdx.x / 64] = f_acc;
	__syncthreads();
	return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

template <int RD>
__global__ void __launch_bounds__(256)
robust_chi2_first_kernel(TRobustParams t, int64_t n_edges, const double *__restrict__ p_sigma_inv, const double *__restrict__ p_error,
	double *p_partial)
{
	__shared__ double p_omega_tile[robust_TILE_EDGES * (RD * RD | 1)], p_err_tile[robust_TILE_EDGES * (RD | 1)];
	const int64_t n_stride = int64_t(gridDim.x) * 256;
	const int n_wave = threadIdx.x / 64, n_lane = threadIdx.x % 64;
	double f_acc = 0;
	for(int64_t n_base = int64_t(blockIdx.x) * 256; n_base < n_edges; n_base += n_stride) {
		for(int j = 0; j < 4; ++ j) {
			const int64_t n_first = n_base + j * robust_TILE_EDGES;
			if(n_first >= n_edges)
				break; // (the same for every thread)
			const int n_here = (n_edges - n_first < robust_TILE_EDGES)? int(n_edges - n_first) : int(robust_TILE_EDGES);
			load_through_tile<RD, 256>(p_err_tile, p_error + n_first * RD, n_here);
			load_through_tile<RD * RD, 256>(p_omega_tile, p_sigma_inv + n_first * RD * RD, n_here);
			__syncthreads();
			if(n_wave == j && n_lane < n_here) {
				double err[RD];
				#pragma unroll
				for(int k = 0; k < RD; ++ k)
					err[k] = p_err_tile[n_lane * (RD | 1) + k];
				const double s = sqrt(robust_quadratic_form<RD>(p_omega_tile + n_lane * (RD * RD | 1), err)) / t.f_scale;
				f_acc += 2 * (t.f_scale * t.f_scale) * robust_rho(t.n_kernel, t.f_param, s);
			}
			__syncthreads(); // (the tiles are used again)
		}
	}
	f_acc = robust_workgroup_sum(f_acc);
	if(threadIdx.x == 0)
		p_partial[blockIdx.x] = f_acc;
}

__global__ void __launch_bounds__(256)
robust_chi2_second_kernel(const double *__restrict__ p_partial, int n_partials, double *p_out)
{
	double f_acc = 0;
	for(int i = threadIdx.x; i < n_partials; i += 256)
		f_acc += p_partial[i];
	f_acc = robust_workgroup_sum(f_acc);
	if(threadIdx.x == 0)
		*p_out = f_acc;
}

void robust_chi2_enqueue(const slampp_hip_robust &r_spec, int64_t n_edges, int rd, const double *p_sigma_inv,
	const double *p_error, double *p_partials, double *p_out, hipStream_t stream)
{
	const int n_groups = int(std::min<int64_t>(reduce_MAX_PARTIALS, std::max<int64_t>(1, (n_edges + 255) / 256))); // (of n_edges alone)
	const TRobustParams t = { r_spec.n_kernel, r_spec.n_basis, r_spec.f_scale, r_spec.f_param };
#define LAUNCH_CHI2(RD) case RD: hipLaunchKernelGGL((robust_chi2_first_kernel<RD>), dim3(n_groups), dim3(256), 0, stream, t, n_edges, \
		p_sigma_inv, p_error, p_partials); break
	switch(rd) {
	LAUNCH_CHI2(1); LAUNCH_CHI2(2); LAUNCH_CHI2(3); LAUNCH_CHI2(4); LAUNCH_CHI2(5); LAUNCH_CHI2(6); LAUNCH_CHI2(7); LAUNCH_CHI2(8);
	default: throw std::domain_error("robust: edge sets with rd <= 8");
	}
#undef LAUNCH_CHI2
	hipLaunchKernelGGL(robust_chi2_second_kernel, dim3(1), dim3(256), 0, stream, p_partials, n_groups, p_out);
	SLAMPP_HIP_CHECK(hipGetLastError());
}

} // namespace slampp
