// schur_resolve.hip -- another right-hand side with what a Schur solve left on the device (slampp_hip_solve_again in Schur
// mode): its kernels and schur_resolve_enqueue, which drives them.  With W_o = U_o C_p^-1, C^-1 and the factor of S kept:
//   r    = eta_c - sum over the observations o of camera c of W_o eta_p(o)      (schur_rhs_kernel of schur.hip, after
//                                                                                schur_resolve_init_kernel has put eta_c in place)
//   dx   = S^-1 r       the dense or the sparse factor's substitutions, or -- after a covariance call that inverted the dense
//                       reduced system in place of its factor -- the product with that inverse (schur_resolve_symv_kernel)
//   dl_p = C_p^-1 eta_p - sum over the cameras c of landmark p of W_(c,p)^T dx_c  (schur_resolve_points_kernel)
// Lambda's values are not read: the reference's counterpart is cholmod_solve on a kept factor
// (LinearSolver_CholMod.cpp:322-347) inside CLinearSolver_Schur's steps 8-13 (LinearSolver_Schur.h:1830-1886).
// Every sum runs in a fixed order.
#include "schur_state.h"
#include "dense_chol.h"

#include <algorithm>

namespace slampp {

// eta_c to where the reduced right-hand side is built: a vector of its own (p_r), or row ld - 1 of the dense factor
__global__ void __launch_bounds__(256)
schur_resolve_init_kernel(const double *__restrict__ eta, int n, double *S, int ld, double *p_r)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if(i < n) {
		if(p_r)
			p_r[i] = eta[i];
		else
			S[size_t(ld - 1) + size_t(i) * ld] = eta[i];
	}
}

// dx = Z r for the symmetric Z = S^-1 whose lower triangle is stored (dense_inverse_from_factor); one wave per row, lane l
// takes columns l, l + 64, ...
__global__ void __launch_bounds__(64)
schur_resolve_symv_kernel(const double *__restrict__ Z, int ld, int n, const double *__restrict__ r, double *dx)
{
	const int i = blockIdx.x, lane = threadIdx.x;
	double sum = 0;
	for(int j = lane; j < n; j += 64)
		sum += ((j <= i)? Z[size_t(i) + size_t(j) * ld] : Z[size_t(j) + size_t(i) * ld]) * r[j];
	#pragma unroll
	for(int m = 1; m < 64; m <<= 1)
		sum += __shfl_xor(sum, m);
	if(lane == 0)
		dx[i] = sum;
}

// one thread per landmark: dl_p (in place of eta_p), and dx copied to the camera part of the vector
template <int DC, int DP>
__global__ void __launch_bounds__(256)
schur_resolve_points_kernel(const int64_t *__restrict__ ptr, const int32_t *__restrict__ brow, int64_t nc, int64_t np, int n,
	const double *__restrict__ Cinv, const double *__restrict__ W, const double *__restrict__ dx, double *out)
{
	const int64_t gid = int64_t(blockIdx.x) * 256 + threadIdx.x;
	if(gid < np) {
		const int64_t pt = gid, k0 = ptr[nc + pt], n_cams = ptr[nc + pt + 1] - k0 - 1; // (the diagonal block is the column's last)
		const int64_t o0 = k0 - ptr[nc] - pt; // observations before this landmark's
		double l[DP], v[DP];
		#pragma unroll
		for(int t = 0; t < DP; ++ t)
			l[t] = out[n + pt * DP + t];
		#pragma unroll
		for(int r = 0; r < DP; ++ r) {
			double s = 0;
			#pragma unroll
			for(int t = 0; t < DP; ++ t)
				s += Cinv[pt * (DP * DP) + r + t * DP] * l[t];
			v[r] = s;
		}
		for(int64_t j = 0; j < n_cams; ++ j) {
			const double *Wo = W + (o0 + j) * (DC * DP), *x = dx + int64_t(brow[k0 + j]) * DC;
			#pragma unroll
			for(int t = 0; t < DP; ++ t) {
				double s = 0;
				#pragma unroll
				for(int i = 0; i < DC; ++ i)
					s += Wo[i + t * DC] * x[i];
				v[t] -= s;
			}
		}
		#pragma unroll
		for(int t = 0; t < DP; ++ t)
			out[n + pt * DP + t] = v[t];
	}
	if(gid < n)
		out[gid] = dx[gid];
}

void schur_resolve_enqueue(slampp_hip_solver &s, double *rhs, bool b_from_covariance)
{
	CSchurState &S = *s.p_schur;
	hipStream_t st = s.stream;
	const int ld = S.Npad, n = S.N;
	// where the factor is: the inner sparse solver's, the dense one in d_S, or -- after a covariance call on the dense reduced
	// system, whose inversion overwrites the factor -- the dense inverse in d_m_Z
	const bool b_sparse = b_from_covariance? S.b_cov_sparse : S.b_reduced_sparse;
	const bool b_inverse = b_from_covariance && !S.b_cov_sparse;
	double *p_r = 0;
	if(b_sparse)
		p_r = S.d_in_buf.p() + size_t(S.n_in_blocks) * S.DC * S.DC;
	else if(b_inverse) {
		S.d_z.Alloc(size_t(ld));
		S.d_x.Alloc(size_t(ld));
		p_r = S.d_z.p();
	}
	s.Phase_Begin("resolve_rhs");
	hipLaunchKernelGGL(schur_resolve_init_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, st, rhs, n, S.d_S.p(), ld, p_r);
	schur_reduced_rhs_launch(S, rhs, S.d_S.p(), p_r, st);
	s.Phase_End();
	const double *p_dx;
	if(b_sparse) {
		s.Phase_Begin("reduced_sparse");
		S.p_inner->p_flag_shared = s.d_flag.p();
		S.p_inner->Enqueue_Sparse(0, p_r, false);
		s.Phase_End();
		p_dx = p_r;
	} else {
		s.Phase_Begin("dense_solve");
		if(b_inverse)
			hipLaunchKernelGGL(schur_resolve_symv_kernel, dim3(unsigned(n)), dim3(64), 0, st, S.d_m_Z.p(), ld, n, p_r, S.d_x.p());
		else {
			dense_forwardsolve(S.d_S.p(), ld, S.d_invdiag.p(), st);
			dense_backsolve(S.d_S.p(), ld, n, S.d_invdiag.p(), S.d_z.p(), S.d_x.p(), st);
		}
		s.Phase_End();
		p_dx = S.d_x.p();
	}
	s.Phase_Begin("backsubst");
	schur_dispatch(S.DC, S.DP, [&](auto dc, auto dp) {
		hipLaunchKernelGGL((schur_resolve_points_kernel<dc(), dp()>), dim3(unsigned((std::max<int64_t>(S.np, n) + 255) / 256)), dim3(256),
			0, st, S.d_ptr.p(), S.d_brow.p(), S.nc, S.np, n, S.d_Cinv.p(), S.d_W.p(), p_dx, rhs);
	});
	s.Phase_End();
	SLAMPP_HIP_CHECK(hipGetLastError());
}

} // namespace slampp
