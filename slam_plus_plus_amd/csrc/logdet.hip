// logdet.hip -- log det Lambda = 2 sum log L_ii from the factor that is already on the device (slampp_hip_logdet).  A unit of
// its own: tests/test_abi.py pins the register allocation of the dense kernels, which has moved before when unrelated
// kernels joined their translation unit.
//
// Two launches, shaped like the dot product of multiply.hip: the first takes one item per lane -- a scalar pivot of the
// factor (through the table of logdet_tables.h, or straight off the diagonal of the dense reduced camera system), or a
// landmark of a Schur-mode system, whose d_p x d_p block C_p is factored in registers -- and leaves one partial sum of
// log(pivot) per workgroup; the second adds the partials, doubles the sum and writes it, or NaN where the handle's
// not-positive-definite flag is raised.  A landmark's lane contributes the sum of log of its own pivots, i.e. half of
// log det C_p, so that everything is doubled in one place.  The number of workgroups follows from the number of items
// alone, the wave sums by a fixed shuffle tree, the waves of a workgroup meet in LDS in wave order and the partials are added
// in a fixed order: no atomics, the same call gives the same bits.
#include "logdet.h"
#include "multiply.h"
#include "schur_state.h"

#include <algorithm>

namespace slampp {

namespace {

__device__ __forceinline__ double logdet_workgroup_sum(double f_acc) // 256 threads; the result in every thread
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

// sum of log of the Cholesky pivots of a D x D block (column-major; the upper triangle is read, as spd_inverse() does
// where the solve factors the same block); a pivot that is not positive gives NaN or -inf
template <int D>
__device__ __forceinline__ double small_chol_log_pivots(const double *__restrict__ a)
{
	double L[D][D], f_sum = 0;
	#pragma unroll
	for(int j = 0; j < D; ++ j) {
		double s = a[j + j * D];
		#pragma unroll
		for(int k = 0; k < D; ++ k)
			if(k < j) s -= L[j][k] * L[j][k];
		const double d = sqrt(s);
		L[j][j] = d;
		f_sum += log(d);
		#pragma unroll
		for(int i = 0; i < D; ++ i) {
			if(i > j) {
				double t = a[j + i * D]; // element (j, i) of the upper triangle = (i, j)
				#pragma unroll
				for(int k = 0; k < D; ++ k)
					if(k < j) t -= L[i][k] * L[j][k];
				L[i][j] = t / d;
			}
		}
	}
	return f_sum;
}

// DP = 0: no landmarks
template <int DC, int DP>
__global__ void __launch_bounds__(256)
logdet_first_kernel(TLogdetSources t, double *partial)
{
	const int64_t n_diag_end = t.n_table + t.n_diag, n_total = n_diag_end + ((DP)? t.n_points : 0);
	const int64_t n_stride = int64_t(gridDim.x) * 256;
	double f_acc = 0;
	for(int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n_total; i += n_stride) {
		if(i < t.n_table) {
			const int64_t n_entry = t.p_table[i];
			f_acc += log((n_entry >= 0)? t.p_L[n_entry] : t.p_dense[(-1 - n_entry) * (t.n_dense_ld + 1)]);
		} else if(i < n_diag_end)
			f_acc += log(t.p_diag[(i - t.n_table) * (t.n_diag_ld + 1)]);
		else if constexpr(DP > 0) {
			// (where C_p sits in the packed values: as schur_point_inverse_kernel finds it -- a landmark's block column
			// holds its observations' U blocks and then C_p; the camera-camera blocks come before all of them)
			const int64_t pt = i - n_diag_end;
			const int64_t n_ublock_base = t.p_ptr[t.n_cams] * (DC * DC);
			const int64_t o1 = t.p_ptr[t.n_cams + pt + 1] - t.p_ptr[t.n_cams] - (pt + 1);
			const double *C = t.p_values + n_ublock_base + o1 * (DC * DP) + pt * (DP * DP);
			double c[DP * DP];
			#pragma unroll
			for(int k = 0; k < DP * DP; ++ k)
				c[k] = C[k];
			f_acc += small_chol_log_pivots<DP>(c);
		}
	}
	f_acc = logdet_workgroup_sum(f_acc);
	if(threadIdx.x == 0)
		partial[blockIdx.x] = f_acc;
}

__global__ void __launch_bounds__(256)
logdet_second_kernel(const double *__restrict__ partial, int n_partials, const int *__restrict__ p_flag, double *out)
{
	double f_acc = 0;
	for(int i = threadIdx.x; i < n_partials; i += 256)
		f_acc += partial[i];
	f_acc = logdet_workgroup_sum(f_acc);
	if(threadIdx.x == 0)
		*out = (p_flag && *p_flag)? __builtin_nan("") : 2 * f_acc;
}

} // anonymous namespace

void logdet_enqueue(const TLogdetSources &r_src, double *p_partials, const int *p_flag, double *p_out, hipStream_t stream)
{
	const int64_t n_total = r_src.n_table + r_src.n_diag + r_src.n_points;
	const int n_groups = int(std::min<int64_t>(reduce_MAX_PARTIALS, std::max<int64_t>(1, (n_total + 1023) / 1024))); // (of the item count alone)
	if(r_src.n_points > 0) {
		schur_dispatch(r_src.n_dc, r_src.n_dp, [&](auto t_dc, auto t_dp) {
			hipLaunchKernelGGL((logdet_first_kernel<decltype(t_dc)::value, decltype(t_dp)::value>), dim3(n_groups), dim3(256), 0,
				stream, r_src, p_partials);
		});
	} else
		hipLaunchKernelGGL((logdet_first_kernel<0, 0>), dim3(n_groups), dim3(256), 0, stream, r_src, p_partials);
	hipLaunchKernelGGL(logdet_second_kernel, dim3(1), dim3(256), 0, stream, p_partials, n_groups, p_flag, p_out);
	SLAMPP_HIP_CHECK(hipGetLastError());
}

} // namespace slampp
