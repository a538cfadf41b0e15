// schur_marginals.hip -- block diagonal of the covariance Lambda^-1 of a BA system from its Schur complement:
//   cameras    Sigma_cc = blocks (c, c) of Z = S^-1
//   landmarks  Sigma_pp = C_p^-1 + sum over the cameras a, b observing p of W_a^T Z(a,b) W_b,   W_o = U_o C_p^-1
// which is what CSchurComplement_Marginals::Schur_Marginals computes
// (/root/reference/include/slam/BAMarginals.h:579-806: Dinv + (R^-T U Dinv)^T (R^-T U Dinv) with S = R^T R, and the
// diagonal blocks of S^-1 by the recursive formula).  Z is dense here (dense_inverse.hip): only its lower triangle
// and the whole of its diagonal 64 x 64 tiles are valid, element (i, j) is read as (max, min).
// The landmark kernel is a gather: k (k + 1) / 2 blocks of Z per landmark with k observations, DC column segments
// each; neighbouring landmarks see neighbouring cameras, so most of them come out of L2.
// With the reduced system factored by the sparse block path, Z is the sparse inverse subset on its factor's pattern instead.
// This file holds the gather kernels and schur_enqueue_marginals, which drives them behind the reduced system's
// factorization (schur.hip: schur_marginals_sparse_factor, schur_marginals_dense_inverse).
#include "schur_state.h"

namespace slampp {

// N contiguous doubles with 16-byte loads where the address allows it (blocks of 6 x 6 and 6 x 3 doubles start at
// multiples of 16 bytes; odd sizes end with one 8-byte load)
template <int N>
__device__ __forceinline__ void load_block(double (&r_dst)[N], const double *__restrict__ p_src)
{
	typedef double v2f64 __attribute__((ext_vector_type(2)));
	if((reinterpret_cast<uintptr_t>(p_src) & 15) == 0) {
		#pragma unroll
		for(int i = 0; i + 1 < N; i += 2) {
			const v2f64 v = *reinterpret_cast<const v2f64*>(p_src + i);
			r_dst[i] = v.x;
			r_dst[i + 1] = v.y;
		}
		if(N & 1)
			r_dst[N - 1] = p_src[N - 1];
	} else {
		#pragma unroll
		for(int i = 0; i < N; ++ i)
			r_dst[i] = p_src[i];
	}
}

template <int DC>
__global__ void schur_cam_cov_kernel(int64_t nc, const double *__restrict__ Z, int ld, double *out)
{
	const int64_t gid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
	if(gid >= nc * (DC * DC))
		return;
	const int64_t c = gid / (DC * DC);
	const int e = int(gid - c * (DC * DC)), r = e % DC, q = e / DC;
	const int hi = (r > q)? r : q, lo = (r > q)? q : r;
	out[gid] = Z[size_t(c * DC + hi) + size_t(c * DC + lo) * ld];
}

template <int DC, int DP>
__global__ void __launch_bounds__(128)
schur_point_cov_kernel(const int64_t *__restrict__ ptr, const int32_t *__restrict__ brow, int64_t nc, int64_t np,
	const double *__restrict__ W, const double *__restrict__ Cinv, const double *__restrict__ Z, int ld, double *out)
{
	const int64_t pt = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
	if(pt >= np)
		return;
	const int64_t k0 = ptr[nc + pt], k1 = ptr[nc + pt + 1] - 1; // the last block of the column is C_p itself
	const int64_t o0 = k0 - ptr[nc] - pt;
	double cov[DP * DP];
	#pragma unroll
	for(int i = 0; i < DP * DP; ++ i)
		cov[i] = Cinv[pt * (DP * DP) + i];
	for(int64_t a = k0; a < k1; ++ a) {
		const int64_t ca = brow[a];
		double wa[DC * DP];
		load_block<DC * DP>(wa, W + (o0 + (a - k0)) * (DC * DP));
		for(int64_t b = k0; b <= a; ++ b) { // block rows ascend inside a column: cb <= ca, the lower triangle of Z
			const int64_t cb = brow[b];
			double wb[DC * DP], t[DC * DP];
			load_block<DC * DP>(wb, W + (o0 + (b - k0)) * (DC * DP));
			#pragma unroll
			for(int i = 0; i < DC * DP; ++ i)
				t[i] = 0;
			#pragma unroll
			for(int q = 0; q < DC; ++ q) {
				double zc[DC]; // column q of the block: contiguous below the diagonal block, (max, min) inside it
				if(a == b) {
					#pragma unroll
					for(int r = 0; r < DC; ++ r) {
						const int hi = (r > q)? r : q, lo = (r > q)? q : r;
						zc[r] = Z[size_t(ca * DC + hi) + size_t(ca * DC + lo) * ld];
					}
				} else
					load_block<DC>(zc, Z + size_t(ca * DC) + size_t(cb * DC + q) * ld);
				#pragma unroll
				for(int r = 0; r < DC; ++ r) {
					#pragma unroll
					for(int j = 0; j < DP; ++ j)
						t[r + j * DC] += zc[r] * wb[q + j * DC];
				}
			}
			#pragma unroll
			for(int j = 0; j < DP; ++ j) {
				#pragma unroll
				for(int i = 0; i < DP; ++ i) {
					double sum = 0;
					#pragma unroll
					for(int r = 0; r < DC; ++ r)
						sum += wa[r + i * DC] * t[r + j * DC];
					cov[i + j * DP] += sum;
					if(a != b)
						cov[j + i * DP] += sum; // the mirrored pair (b, a) contributes the transpose
				}
			}
		}
	}
	#pragma unroll
	for(int i = 0; i < DP * DP; ++ i)
		out[pt * (DP * DP) + i] = cov[i];
}

// ---- the same from the sparse inverse subset (sparse_inverse.hip): Z is laid out like the factor of the reduced system,
// in its elimination order; where a block sits and whether it is stored transposed comes from host-built tables ----
template <int DC>
__global__ void schur_cam_cov_sparse_kernel(int64_t nc, const int64_t *__restrict__ cam_zoff, const double *__restrict__ Z, double *out)
{
	const int64_t gid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
	if(gid >= nc * (DC * DC))
		return;
	const int64_t c = gid / (DC * DC);
	out[gid] = Z[cam_zoff[c] + (gid - c * (DC * DC))]; // diagonal blocks are stored whole
}

template <int DC, int DP>
__global__ void __launch_bounds__(128)
schur_point_cov_sparse_kernel(const int64_t *__restrict__ ptr, int64_t nc, int64_t np, const int64_t *__restrict__ pair_ptr,
	const int64_t *__restrict__ pair_tab, const double *__restrict__ W, const double *__restrict__ Cinv,
	const double *__restrict__ Z, double *out)
{
	const int64_t pt = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
	if(pt >= np)
		return;
	const int64_t k0 = ptr[nc + pt], k1 = ptr[nc + pt + 1] - 1;
	const int64_t o0 = k0 - ptr[nc] - pt;
	const int64_t *tab = pair_tab + pair_ptr[pt];
	double cov[DP * DP];
	#pragma unroll
	for(int i = 0; i < DP * DP; ++ i)
		cov[i] = Cinv[pt * (DP * DP) + i];
	for(int64_t a = k0; a < k1; ++ a) {
		double wa[DC * DP];
		load_block<DC * DP>(wa, W + (o0 + (a - k0)) * (DC * DP));
		for(int64_t b = k0; b <= a; ++ b) {
			const int64_t ia = a - k0, ib = b - k0;
			const int64_t ent = tab[ia * (ia + 1) / 2 + ib]; // block Z(cam_a, cam_b): offset * 2 + stored transposed
			const bool b_tr = ent & 1;
			double wb[DC * DP], zb[DC * DC], t[DC * DP];
			load_block<DC * DC>(zb, Z + (ent >> 1)); // a thread's scattered loads are paid per instruction: 16 bytes each
			load_block<DC * DP>(wb, W + (o0 + ib) * (DC * DP));
			#pragma unroll
			for(int i = 0; i < DC * DP; ++ i)
				t[i] = 0;
			#pragma unroll
			for(int q = 0; q < DC; ++ q) {
				#pragma unroll
				for(int r = 0; r < DC; ++ r) {
					const double z = b_tr? zb[q + r * DC] : zb[r + q * DC];
					#pragma unroll
					for(int j = 0; j < DP; ++ j)
						t[r + j * DC] += z * wb[q + j * DC];
				}
			}
			#pragma unroll
			for(int j = 0; j < DP; ++ j) {
				#pragma unroll
				for(int i = 0; i < DP; ++ i) {
					double sum = 0;
					#pragma unroll
					for(int r = 0; r < DC; ++ r)
						sum += wa[r + i * DC] * t[r + j * DC];
					cov[i + j * DP] += sum;
					if(a != b)
						cov[j + i * DP] += sum;
				}
			}
		}
	}
	#pragma unroll
	for(int i = 0; i < DP * DP; ++ i)
		out[pt * (DP * DP) + i] = cov[i];
}

// the block diagonal gathered from the inverse subset in d_m_Zs (S.b_cov_sparse) or from the dense inverse in d_m_Z; either
// output may be null
static void schur_marginals_gather(CSchurState &S, double *cam_cov, double *point_cov, hipStream_t stream)
{
	schur_dispatch(S.DC, S.DP, [&](auto dc, auto dp) {
		constexpr int DC = dc(), DP = dp();
		const dim3 cam_grid(unsigned((S.nc * DC * DC + 255) / 256)), point_grid(unsigned((S.np + 127) / 128));
		if(cam_cov && S.b_cov_sparse)
			hipLaunchKernelGGL((schur_cam_cov_sparse_kernel<DC>), cam_grid, dim3(256), 0, stream,
				S.nc, S.d_cam_zoff.p(), S.d_m_Zs.p(), cam_cov);
		else if(cam_cov)
			hipLaunchKernelGGL((schur_cam_cov_kernel<DC>), cam_grid, dim3(256), 0, stream, S.nc, S.d_m_Z.p(), S.Npad, cam_cov);
		if(point_cov && S.b_cov_sparse)
			hipLaunchKernelGGL((schur_point_cov_sparse_kernel<DC, DP>), point_grid, dim3(128), 0, stream,
				S.d_ptr.p(), S.nc, S.np, S.d_pair_ptr.p(), S.d_pair_tab.p(), S.d_W.p(), S.d_Cinv.p(), S.d_m_Zs.p(), point_cov);
		else if(point_cov)
			hipLaunchKernelGGL((schur_point_cov_kernel<DC, DP>), point_grid, dim3(128), 0, stream,
				S.d_ptr.p(), S.d_brow.p(), S.nc, S.np, S.d_W.p(), S.d_Cinv.p(), S.d_m_Z.p(), S.Npad, point_cov);
	});
}

// Block diagonal of Lambda^-1: the reduced system is assembled into a dense buffer of its own whatever way the solves
// factor it, factored, inverted on the matrix cores, then gathered per landmark -- or, where the solves factor it by the
// sparse block path, assembled and factored there, and the blocks of S^-1 on the factor's pattern are gathered
// (sparse_inverse.hip).  Landmark shards: S is summed over the ranks; every rank then writes the covariances of its own
// landmarks.
void schur_enqueue_marginals(slampp_hip_solver &s, const double *p_values_dev, double *p_cam_cov_dev, double *p_point_cov_dev)
{
	schur_invalidate_previous(s.p_schur); // C^-1, W (and the packed reduced system) are recomputed from these values
	CSchurState &S = *s.p_schur;
	// decided as for a solve: with the sparse reduced system the covariances go through the sparse inverse subset
	if(s.p_allreduce && (S.p_union_fn != s.p_allreduce || S.p_union_context != s.p_allreduce_context))
		schur_agree_on_union(s, S);
	if(!S.b_reduced_decided)
		schur_setup_reduced(s, S);
	S.b_cov_sparse = S.b_reduced_sparse && s.n_marginals_dense == 0 && schur_setup_sparse_marginals(s, S);
	if(S.b_cov_sparse) {
		schur_marginals_sparse_factor(s, S, p_values_dev);
		s.Phase_Begin("marginals_inverse");
		sparse_inverse_enqueue(*S.p_sinv, S.p_inner->plan, S.p_inner->d_L.p(), S.p_inner->d_Linv.p(), S.d_m_Zs.p(), s.stream);
		s.Phase_End();
	} else
		schur_marginals_dense_inverse(s, S, p_values_dev);
	S.b_cov_z_valid = true; // (either way the inverse is of these values)
	s.Phase_Begin("marginals_gather");
	schur_marginals_gather(S, p_cam_cov_dev, p_point_cov_dev, s.stream);
	s.Phase_End();
	SLAMPP_HIP_CHECK(hipGetLastError());
}

} // namespace slampp
