// linearize.h -- the two ends of a Gauss-Newton / LM iteration on the device (linearize.hip): every edge's error and
// Jacobians from the vertex states, the states moved on their manifold by a solution, and chi^2
#pragma once

#include "solver.h"

namespace slampp {

enum { linearize_TILE_EDGES = 64 }; // edges of a workgroup: a lane each, their outputs staged in LDS and written as whole lines

// error and Jacobians of every edge of the set (n_edge_type: SLAMPP_HIP_EDGE_*, matching the view's dimensions: the caller
// checks) into the arrays the assembly reads; p_params only for SLAMPP_HIP_EDGE_P2C_XYZ.  p_J0 and p_J1 both null: the
// errors alone, to the bits of the call that writes all three (edge_errors of the C ABI).  Throws.
void linearize_enqueue(int n_edge_type, const TAsmEdgeView &r_edges, const double *p_state, const double *p_measurement,
	const double *p_params, double *p_J0, double *p_J1, double *p_error, hipStream_t stream);

// out = state (+) f_scale dx on block columns [n_first, n_last) (n_vertex_type: SLAMPP_HIP_VERTEX_*; the dimensions fit: the
// caller checks); p_cumsum: the block columns' scalar offsets on the device; out == state or disjoint.  Throws.
void state_plus_enqueue(int n_vertex_type, const int64_t *p_cumsum, int64_t n_first, int64_t n_last, const double *p_state,
	const double *p_dx, double f_scale, double *p_out, hipStream_t stream);

// *p_out = sum over the edges of w_e err_e^T Omega_e err_e in two passes whose shape depends on n_edges alone (p_weight may
// be null); p_partials: reduce_MAX_PARTIALS doubles of workspace.  Throws.
void chi2_enqueue(int64_t n_edges, int rd, const double *p_sigma_inv, const double *p_error, const double *p_weight,
	double *p_partials, double *p_out, hipStream_t stream);

} // namespace slampp
