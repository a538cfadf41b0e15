// linearize.hip -- the two ends of a Gauss-Newton / LM iteration that the assembly, the damping and the solve left on the host:
//   linearize   every edge's error and Jacobians from the vertex states  (the reference's Calculate_Jacobians_Expectation_Error
//               of CEdgePose2D, CEdgePose3D, CEdgeP2C3D, CEdgePoseLandmark2D, CEdgePoseLandmark3D and CEdgeP2SC3D: SE2_Types.h:308-318, 562-573,
//               SE3_Types.h:265-287, 569-587, BA_Types.h:494-505, 796-811),
//               written where assembly.hip reads them;
//   state_plus  x <- x (+) s dx on the vertices' manifolds  (Operator_Plus / Operator_Minus of CVertexPose2D, CVertexPose3D,
//               CVertexCam, CVertexXYZ, which PushValuesInGraphSystem runs over the vertex pool);
//   chi2        sum of w err^T Sigma^-1 err  (f_Chi_Squared_Error summed over the edge pool).
// The arithmetic of one edge or vertex is linearize_math.h; this file is the memory traffic around it.  All of it is HBM-bound
// (an SE(3) edge gathers 18 doubles and writes 78), plain fp64, no atomics: the same call twice gives the same bits.
#include "linearize.h"
#include "linearize_math.h"
#include "multiply.h"

#include <algorithm>

namespace slampp {

// the row of edge_type_shape (linearize.h) as compile-time constants; NP: the parameters per block column of vertex 0
template <int n_edge_type> struct TEdgeShape {
	static_assert(edge_type_shape(n_edge_type).b_known, "no such edge type");
	enum { D0 = edge_type_shape(n_edge_type).d0, D1 = edge_type_shape(n_edge_type).d1, RD = edge_type_shape(n_edge_type).rd,
		MD = edge_type_shape(n_edge_type).n_measurement, NP = edge_type_shape(n_edge_type).n_params };
};

// The lanes of the workgroup hold N doubles each for n_here consecutive edges; in memory those are one run of n_here * N
// doubles.  A lane storing its own N would walk memory with a stride of 8 N bytes (288 for an SE(3) Jacobian: every store
// instruction touches 64 lines).  Instead the values cross through an LDS tile, one row per edge, and leave as consecutive
// doubles of consecutive lanes.  A tile row is N | 1 doubles: the side that walks down a tile column (a lane per row) has an
// odd stride in doubles and spreads over the banks, as in half_export_kernel ("The transposes").
template <int N>
__device__ __forceinline__ void store_through_tile(double *p_tile, const double (&v)[N], bool b_mine, double *__restrict__ p_dst,
	int n_here)
{
	enum { STRIDE = N | 1 };
	if(b_mine) {
		#pragma unroll
		for(int k = 0; k < N; ++ k)
			p_tile[threadIdx.x * STRIDE + k] = v[k];
	}
	__syncthreads();
	for(int i = threadIdx.x; i < n_here * N; i += linearize_TILE_EDGES)
		p_dst[i] = p_tile[(i / N) * STRIDE + i % N];
	__syncthreads(); // (the tile is used again)
}

// a lane per edge, linearize_TILE_EDGES edges per workgroup.  Nothing an edge computes depends on its neighbours in the tile:
// a call on the first n edges of a set gives those edges the bits of the call on the whole set.
// b_jacobians = false: the errors alone (the reference's f_Chi_Squared_Error evaluates no more), by the same arithmetic --
// the Jacobians are not stored, p_J0 and p_J1 are not read, and what only they need is left to the compiler to drop.
template <int n_edge_type, bool b_jacobians>
__global__ void __launch_bounds__(linearize_TILE_EDGES)
linearize_kernel(int64_t n_edges, const int64_t *__restrict__ p_off0, const int64_t *__restrict__ p_off1,
	const int64_t *__restrict__ p_vertex0, const double *__restrict__ p_state, const double *__restrict__ p_measurement,
	const double *__restrict__ p_params, double *__restrict__ p_J0, double *__restrict__ p_J1, double *__restrict__ p_error)
{
	typedef TEdgeShape<n_edge_type> S;
	enum { D0 = S::D0, D1 = S::D1, RD = S::RD, MD = S::MD, NP = S::NP, N0 = RD * D0, N1 = RD * D1,
		N_MAX = (!b_jacobians)? RD : (N0 > N1)? N0 : N1 };
	__shared__ double p_tile[linearize_TILE_EDGES * (N_MAX | 1)];
	const int64_t n_first = int64_t(blockIdx.x) * linearize_TILE_EDGES, e = n_first + threadIdx.x;
	const int n_here = (n_edges - n_first < linearize_TILE_EDGES)? int(n_edges - n_first) : int(linearize_TILE_EDGES);
	const bool b_mine = e < n_edges;
	double J0[N0], J1[N1], err[RD];
	if(b_mine) {
		double x0[D0], x1[D1], z[MD];
		const double *p_x0 = p_state + p_off0[e], *p_x1 = p_state + p_off1[e], *p_z = p_measurement + e * MD;
		#pragma unroll
		for(int i = 0; i < D0; ++ i)
			x0[i] = p_x0[i];
		#pragma unroll
		for(int i = 0; i < D1; ++ i)
			x1[i] = p_x1[i];
		#pragma unroll
		for(int i = 0; i < MD; ++ i)
			z[i] = p_z[i];
		if(n_edge_type == SLAMPP_HIP_EDGE_SE2)
			lin::edge_se2(x0, x1, z, J0, J1, err);
		else if(n_edge_type == SLAMPP_HIP_EDGE_SE3)
			lin::edge_se3(x0, x1, z, J0, J1, err);
		else if(n_edge_type == SLAMPP_HIP_EDGE_POSE_LANDMARK_2D)
			lin::edge_pose_landmark_2d(x0, x1, z, J0, J1, err);
		else if(n_edge_type == SLAMPP_HIP_EDGE_POSE_LANDMARK_3D)
			lin::edge_pose_landmark_3d(x0, x1, z, J0, J1, err);
		else {
			double k[(NP)? NP : 1];
			const double *p_k = p_params + NP * p_vertex0[e];
			#pragma unroll
			for(int i = 0; i < NP; ++ i)
				k[i] = p_k[i];
			if(n_edge_type == SLAMPP_HIP_EDGE_P2C_XYZ)
				lin::edge_p2c_xyz(x0, x1, z, k, J0, J1, err);
			else
				lin::edge_p2sc_xyz(x0, x1, z, k, J0, J1, err);
		}
	}
	if(b_jacobians) {
		store_through_tile<N0>(p_tile, J0, b_mine, p_J0 + n_first * N0, n_here);
		store_through_tile<N1>(p_tile, J1, b_mine, p_J1 + n_first * N1, n_here);
	}
	store_through_tile<RD>(p_tile, err, b_mine, p_error + n_first * RD, n_here);
}

void linearize_enqueue(int n_edge_type, const TAsmEdgeView &v, const double *p_state, const double *p_measurement,
	const double *p_params, double *p_J0, double *p_J1, double *p_error, hipStream_t stream)
{
	const int64_t n_grid = (v.n_edges + linearize_TILE_EDGES - 1) / linearize_TILE_EDGES;
	if(n_grid < 1 || n_grid > 0x7fffffff)
		throw std::domain_error("linearize: too many edges");
#define LAUNCH_LINEARIZE(T) do { if(p_J0) hipLaunchKernelGGL((linearize_kernel<T, true>), dim3(unsigned(n_grid)), \
		dim3(linearize_TILE_EDGES), 0, stream, v.n_edges, v.p_state_off0, v.p_state_off1, v.p_vertex0, p_state, p_measurement, p_params, \
		p_J0, p_J1, p_error); \
	else hipLaunchKernelGGL((linearize_kernel<T, false>), dim3(unsigned(n_grid)), dim3(linearize_TILE_EDGES), 0, stream, v.n_edges, \
		v.p_state_off0, v.p_state_off1, v.p_vertex0, p_state, p_measurement, p_params, p_J0, p_J1, p_error); } while(0)
	if(!p_J0 != !p_J1)
		throw std::invalid_argument("linearize: one Jacobian array without the other");
	switch(n_edge_type) {
	case SLAMPP_HIP_EDGE_SE2: LAUNCH_LINEARIZE(SLAMPP_HIP_EDGE_SE2); break;
	case SLAMPP_HIP_EDGE_SE3: LAUNCH_LINEARIZE(SLAMPP_HIP_EDGE_SE3); break;
	case SLAMPP_HIP_EDGE_P2C_XYZ: LAUNCH_LINEARIZE(SLAMPP_HIP_EDGE_P2C_XYZ); break;
	case SLAMPP_HIP_EDGE_POSE_LANDMARK_2D: LAUNCH_LINEARIZE(SLAMPP_HIP_EDGE_POSE_LANDMARK_2D); break;
	case SLAMPP_HIP_EDGE_POSE_LANDMARK_3D: LAUNCH_LINEARIZE(SLAMPP_HIP_EDGE_POSE_LANDMARK_3D); break;
	case SLAMPP_HIP_EDGE_P2SC_XYZ: LAUNCH_LINEARIZE(SLAMPP_HIP_EDGE_P2SC_XYZ); break;
	default: throw std::invalid_argument("linearize: unknown edge type");
	}
#undef LAUNCH_LINEARIZE
	SLAMPP_HIP_CHECK(hipGetLastError());
}

// a lane per block column: it reads its vertex' state and step, then writes; out == state is safe (no lane reads what
// another writes), and the columns outside [n_first, n_last) are not touched
template <int n_vertex_type>
__global__ void __launch_bounds__(256)
state_plus_kernel(const int64_t *__restrict__ p_cumsum, int64_t n_first, int64_t n_last, const double *p_state,
	const double *__restrict__ p_dx, double f_scale, double *p_out)
{
	const int64_t v = n_first + int64_t(blockIdx.x) * 256 + threadIdx.x;
	if(v >= n_last)
		return;
	const int64_t n_off = p_cumsum[v];
	if(n_vertex_type == SLAMPP_HIP_VERTEX_EUCLIDEAN) {
		const int d = int(p_cumsum[v + 1] - n_off); // (<= 8: the host checked)
		for(int i = 0; i < d; ++ i)
			p_out[n_off + i] = p_state[n_off + i] + f_scale * p_dx[n_off + i];
	} else {
		enum { D = (n_vertex_type == SLAMPP_HIP_VERTEX_SE2)? 3 : 6 };
		double x[D], dx[D];
		#pragma unroll
		for(int i = 0; i < D; ++ i) {
			x[i] = p_state[n_off + i];
			dx[i] = p_dx[n_off + i];
		}
		if(n_vertex_type == SLAMPP_HIP_VERTEX_SE2)
			lin::plus_se2(x, dx, f_scale, x);
		else
			lin::plus_se3(x, dx, f_scale, x);
		#pragma unroll
		for(int i = 0; i < D; ++ i)
			p_out[n_off + i] = x[i];
	}
}

void state_plus_enqueue(int n_vertex_type, const int64_t *p_cumsum, int64_t n_first, int64_t n_last, const double *p_state,
	const double *p_dx, double f_scale, double *p_out, hipStream_t stream)
{
	if(n_first >= n_last)
		return;
	const int64_t n_grid = (n_last - n_first + 255) / 256;
	if(n_grid > 0x7fffffff)
		throw std::domain_error("state_plus: too many block columns");
#define LAUNCH_PLUS(T) hipLaunchKernelGGL((state_plus_kernel<T>), dim3(unsigned(n_grid)), dim3(256), 0, stream, p_cumsum, n_first, \
	n_last, p_state, p_dx, f_scale, p_out)
	switch(n_vertex_type) {
	case SLAMPP_HIP_VERTEX_EUCLIDEAN: LAUNCH_PLUS(SLAMPP_HIP_VERTEX_EUCLIDEAN); break;
	case SLAMPP_HIP_VERTEX_SE2: LAUNCH_PLUS(SLAMPP_HIP_VERTEX_SE2); break;
	case SLAMPP_HIP_VERTEX_SE3: LAUNCH_PLUS(SLAMPP_HIP_VERTEX_SE3); break;
	default: throw std::invalid_argument("state_plus: unknown vertex type");
	}
#undef LAUNCH_PLUS
	SLAMPP_HIP_CHECK(hipGetLastError());
}

// ---- chi^2: the two passes of dot_enqueue (multiply.hip) with an edge's term in the place of a product ----

__device__ __forceinline__ double chi2_workgroup_sum(double f_acc) // 256 threads; the result in thread 0
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

// a lane per edge computes w err^T Omega err (Omega column-major rd x rd, summed column by column); a lane adds the terms of
// its edges in ascending order, the workgroup adds its lanes' sums in one fixed tree
__global__ void __launch_bounds__(256)
chi2_first_kernel(int64_t n_edges, int rd, const double *__restrict__ p_sigma_inv, const double *__restrict__ p_error,
	const double *__restrict__ p_weight, double *p_partial)
{
	const int64_t n_stride = int64_t(gridDim.x) * 256;
	double f_acc = 0;
	for(int64_t e = int64_t(blockIdx.x) * 256 + threadIdx.x; e < n_edges; e += n_stride) {
		const double *p_omega = p_sigma_inv + e * rd * rd, *p_err = p_error + e * rd;
		double f_term = 0;
		for(int c = 0; c < rd; ++ c) {
			double f_col = 0;
			for(int r = 0; r < rd; ++ r)
				f_col += p_err[r] * p_omega[r + c * rd];
			f_term += f_col * p_err[c];
		}
		f_acc += (p_weight)? p_weight[e] * f_term : f_term;
	}
	f_acc = chi2_workgroup_sum(f_acc);
	if(threadIdx.x == 0)
		p_partial[blockIdx.x] = f_acc;
}

__global__ void __launch_bounds__(256)
chi2_second_kernel(const double *__restrict__ p_partial, int n_partials, double *p_out)
{
	double f_acc = 0;
	for(int i = threadIdx.x; i < n_partials; i += 256)
		f_acc += p_partial[i];
	f_acc = chi2_workgroup_sum(f_acc);
	if(threadIdx.x == 0)
		*p_out = f_acc;
}

void chi2_enqueue(int64_t n_edges, int rd, const double *p_sigma_inv, const double *p_error, const double *p_weight,
	double *p_partials, double *p_out, hipStream_t stream)
{
	const int n_groups = int(std::min<int64_t>(reduce_MAX_PARTIALS, std::max<int64_t>(1, (n_edges + 255) / 256))); // (of n_edges alone)
	hipLaunchKernelGGL(chi2_first_kernel, dim3(n_groups), dim3(256), 0, stream, n_edges, rd, p_sigma_inv, p_error, p_weight, p_partials);
	hipLaunchKernelGGL(chi2_second_kernel, dim3(1), dim3(256), 0, stream, p_partials, n_groups, p_out);
	SLAMPP_HIP_CHECK(hipGetLastError());
}

} // namespace slampp
