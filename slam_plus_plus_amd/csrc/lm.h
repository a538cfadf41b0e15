// lm.h -- the accept / reject and damping rule of the Levenberg-Marquardt loop on the device (lm.hip): the reference's
// CLevenbergMarquardt_Baseline (NonlinearSolver_Lambda_LM.h:151-223) inside the loop of CNonlinearSolver_Lambda_LM::Optimize
// (:915-1115), decided by kernels on a block of scalars in device memory (the indices: SLAMPP_HIP_LM_* in
// include/slampp_hip.h), so that a caller enqueues N iterations and waits once.
#pragma once

#include "solver.h"

namespace slampp {

enum { lm_MAX_SETS = 8, lm_MAX_DIM = 8, lm_TRACE_RECORD = 8 };

// one edge set of the initial damping: Jacobians and Sigma^-1 edge-major, column-major matrices; p_weight may be null
struct TLmDampingSet {
	int64_t n_edges;
	int d0, d1, rd;
	const double *p_J0, *p_J1, *p_sigma_inv, *p_weight;
};

// *p_alpha_out = f_tau max over the edges of all the sets of the largest diagonal entry of w J0^T Omega J0 and of
// w J1^T Omega J1 (f_InitialDamping through f_Max_VertexHessianDiagValue: the maximum starts from 0 and a NaN does not
// enter it).  Two passes shaped like chi2_enqueue, per set; the partial maxima of set i at p_partials + i reduce_MAX_PARTIALS
// (lm_MAX_SETS * reduce_MAX_PARTIALS doubles of workspace).  A maximum does not depend on the order: bit-reproducible.  Throws.
void lm_initial_damping_enqueue(const TLmDampingSet *p_sets, int n_sets, double f_tau, double *p_partials, double *p_alpha_out,
	hipStream_t stream);

// values += f_scale * *p_alpha on the diagonal of the diagonal blocks of block columns [n_first, n_last) (damping_enqueue with
// the damping read from device memory)
void lm_damping_scalar_enqueue(const int64_t *p_off_dim_dev, int64_t n_first, int64_t n_last, const double *p_alpha, double f_scale,
	double *p_values_dev, hipStream_t stream);

// p_lm[DX_DX] = dx^T dx and p_lm[DX_ETA] = dx^T eta in one pass over the two vectors, with the partition and the trees of
// dot_enqueue (of n alone); p_partials: 2 * reduce_MAX_PARTIALS doubles.  Nothing is written once p_lm[STATUS] is not 0.
void lm_gain_enqueue(const double *p_dx, const double *p_eta, int64_t n, double *p_partials, double *p_lm, hipStream_t stream);

// one decision on the block of scalars (one lane); p_flag: the handle's not-positive-definite flag; p_trace may be null
void lm_decide_enqueue(double *p_lm, const double *p_chi_parts, int n_parts, const int *p_flag, double *p_trace, int64_t n_trace,
	hipStream_t stream);

// state = trial where p_lm[ACCEPTED] is not 0; otherwise nothing is written
void lm_commit_enqueue(const double *p_lm, double *p_state, const double *p_trial, int64_t n, hipStream_t stream);

// the scalars at the start of a loop (a kernel: the call is enqueue-only); f_tau > 0: ALPHA = *p_alpha_dev (what
// lm_initial_damping_enqueue left there, which may be p_lm + ALPHA itself), otherwise f_alpha; LAST_ERROR = the sum of the parts
void lm_begin_enqueue(double *p_lm, const double *p_alpha_dev, double f_alpha, const double *p_chi_parts, int n_parts,
	double f_min_dx_norm, int n_max_iterations, int n_extra_on_reject, hipStream_t stream);

} // namespace slampp
