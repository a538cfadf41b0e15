// linearize.h -- the two ends of a Gauss-Newton / LM iteration on the device (linearize.hip): every edge's error and
// Jacobians from the vertex states, the states moved on their manifold by a solution, and chi^2
#pragma once

#include "solver.h"

namespace slampp {

enum { linearize_TILE_EDGES = 64 }; // edges of a workgroup: a lane each, their outputs staged in LDS and written as whole lines

// The one table of the edge types: the vertex dimensions, the residual dimension, the doubles of a measurement and the
// parameters per block column of vertex 0 (0: the type takes no p_params).  b_known is false for a value that is no
// SLAMPP_HIP_EDGE_* (4 among them).  The kernel's template, the launch and the refusals of the C ABI all read it.
struct TEdgeTypeShape {
	bool b_known;
	int d0, d1, rd, n_measurement, n_params;
};

constexpr TEdgeTypeShape edge_type_shape(int n_edge_type)
{
	switch(n_edge_type) {
	case SLAMPP_HIP_EDGE_SE2: return TEdgeTypeShape{true, 3, 3, 3, 3, 0};
	case SLAMPP_HIP_EDGE_SE3: return TEdgeTypeShape{true, 6, 6, 6, 6, 0};
	case SLAMPP_HIP_EDGE_P2C_XYZ: return TEdgeTypeShape{true, 6, 3, 2, 2, 5};
	case SLAMPP_HIP_EDGE_POSE_LANDMARK_2D: return TEdgeTypeShape{true, 3, 2, 2, 2, 0};
	case SLAMPP_HIP_EDGE_POSE_LANDMARK_3D: return TEdgeTypeShape{true, 6, 3, 3, 3, 0};
	case SLAMPP_HIP_EDGE_P2SC_XYZ: return TEdgeTypeShape{true, 6, 3, 3, 3, 6};
	default: return TEdgeTypeShape{false, 0, 0, 0, 0, 0};
	}
}

// error and Jacobians of every edge of the set (n_edge_type: SLAMPP_HIP_EDGE_*, matching the view's dimensions: the caller
// checks) into the arrays the assembly reads; p_params only for the types with parameters in the table above.  p_J0 and p_J1 both null: the
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
