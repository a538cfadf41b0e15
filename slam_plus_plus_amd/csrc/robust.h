// robust.h -- robust kernels on the device (robust.hip): the per-edge weight w(s) of the reference's loss functions
// (include/geometry/RobustLoss.h: Huber :103, Cauchy :153, Tukey :206, Welsch :433) on the bases of its two "robustify" edge
// bases (slam/RobustUtils.h:397-399 the error norm, :531-534 chi^2) and on the Mahalanobis distance, the scaling of an edge
// set's Jacobians and errors by sqrt(w), and the robust cost sum 2 scale^2 rho(s) -- include/slampp_hip.h has the formulas
#pragma once

#include "solver.h"

namespace slampp {

enum { robust_TILE_EDGES = 64, robust_MAX_DIM = 8 }; // edges of a tile: a lane each, their records staged in LDS as whole lines

// p_weight[e] = w(s_e) for the n_edges edges of residual dimension rd (1 to robust_MAX_DIM); p_sigma_inv [n_edges][rd x rd]
// is not read with SLAMPP_HIP_ROBUST_BASIS_ERROR_NORM.  The specification was checked by the caller.  Throws.
void robust_weights_enqueue(const slampp_hip_robust &r_spec, int64_t n_edges, int rd, const double *p_sigma_inv,
	const double *p_error, double *p_weight, hipStream_t stream);

// every element of p_J0 [n_edges][rd x d0], p_J1 [n_edges][rd x d1] and p_error [n_edges][rd] times sqrt(p_weight[its edge]),
// in place.  Throws.
void robust_scale_enqueue(int64_t n_edges, int rd, int d0, int d1, const double *p_weight, double *p_J0, double *p_J1,
	double *p_error, hipStream_t stream);

// *p_out = sum over the edges of 2 scale^2 rho(sqrt(err^T Omega err) / scale) in the two passes of chi2_enqueue (linearize.h):
// the same partition, the same trees; p_partials: reduce_MAX_PARTIALS doubles of workspace.  Throws.
void robust_chi2_enqueue(const slampp_hip_robust &r_spec, int64_t n_edges, int rd, const double *p_sigma_inv,
	const double *p_error, double *p_partials, double *p_out, hipStream_t stream);

} // namespace slampp
