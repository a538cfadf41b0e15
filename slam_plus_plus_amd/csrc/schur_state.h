// schur_state.h -- internal to the Schur units (schur*.hip): the state behind a handle in Schur mode, the one dispatch on
// the block sizes, and every function those units call in each other.  What capi*.hip, solver.hip and group.hip call is
// declared in solver.h.
#pragma once
#include "solver.h"
#include "sparse_inverse.h"
#include "schur_tiles.h"

#include <stdexcept>
#include <type_traits>

namespace slampp {

struct TSchurPairRec { // 24 B: one pair of slampp_hip_schur_marginal_blocks, r <= c in the caller's block columns
	int64_t out;    // offset of its block in the output
	int32_t r, c;   // camera index, or landmark index (0-based among the landmarks)
	int32_t kind;   // bit 0: r is a landmark, bit 1: c is one (a camera and a landmark: the camera is r)
	int32_t b_tr;   // the caller listed (c, r): the block is written transposed
};

struct CSchurState {
	int DC, DP;
	int64_t nc, np, n_obs, n_ablocks, n_sblocks, n_entries;
	int N, Npad;
	CDevArray<int64_t> d_ptr;       // [n+1] block column pointers of Lambda
	CDevArray<int32_t> d_brow;      // [n_blocks]
	CDevArray<int32_t> d_obs_pt;    // [n_obs]
	CDevArray<int64_t> d_sb_ptr;    // [n_sblocks+1]
	CDevArray<int32_t> d_sb_row, d_sb_col;
	CDevArray<int32_t> d_ent_a;     // [n_entries] observation whose W is used
	CDevArray<int64_t> d_ent_uoff;  // [n_entries] offset of the U block of the other observation in the values
	CDevArray<int64_t> d_cam_ptr;   // [nc+1]
	CDevArray<int32_t> d_cam_obs;   // [n_obs] observations of every camera, ascending
	CDevArray<double> d_S, d_W, d_Cinv, d_t, d_invdiag, d_z, d_x;
	// multi-GPU: the all-reduce moves only the blocks of S that are nonzero on some rank
	std::vector<int32_t> h_blk_row, h_blk_col; // this rank's nonzero blocks of S (lower triangle; camera indices)
	slampp_hip_allreduce_fn p_union_fn;        // the callback the union below was agreed through
	void *p_union_context;
	bool b_union_dense;                        // too many cameras for the indicator exchange: reduce the whole buffer
	int64_t n_union;
	CDevArray<int32_t> d_un_row, d_un_col;
	CDevArray<double> d_pack;                  // [n_union DC^2 + N]
	std::vector<int32_t> h_un_row, h_un_col;   // the agreed list, sorted by (column, row)
	// sparse reduced system: S handed to the sparse block path as its own little Lambda
	bool b_reduced_decided, b_reduced_sparse;
	slampp_hip_solver *p_inner;
	int64_t n_in_blocks;
	CDevArray<int64_t> d_sb_dst, d_a_dst;      // where the blocks of S this rank computes / the camera blocks of Lambda sit
	                                           // in the packed upper block-CSC values of the inner solver
	CDevArray<double> d_in_buf;                // [values (n_in_blocks DC^2) | right-hand side (N)]: also what the ranks exchange
	// marginal covariances (own buffers: the factor the last solve left behind stays usable)
	CDevArray<double> d_m_S, d_m_Z, d_m_invdiag, d_m_zero;
	// ... through the sparse inverse subset when the reduced system is factored by the sparse block path
	CSparseInverse *p_sinv;
	bool b_sinv_tried;
	CDevArray<double> d_m_Zs;                  // laid out like the inner solver's factor
	CDevArray<int64_t> d_cam_zoff, d_pair_ptr, d_pair_tab;
	// incremental update of the reduced system (option "schur_incremental"): what the previous solve assembled stays, and
	// a solve that names the landmarks whose blocks changed exchanges their contributions only
	bool b_prev_valid = false;                 // the buffers below describe the values of the last solve
	CDevArray<double> d_A_prev;                // the camera-camera blocks of Lambda of the last solve
	CDevArray<double> d_S_unf;                 // dense reduced system: S as assembled (d_S is factored in place)
	CDevArray<int64_t> d_changed;              // landmarks named for the next solve
	int64_t n_changed = -1;                    // -1: none named (full rebuild)
	CSchurTiles tiles;                         // landmark-major assembly of S (schur_tiles.hip)
	// covariances beyond the block diagonal (schur_covariance.hip): the reduced-system path the last of those calls took,
	// whether the sparse inverse subset of its factor is in d_m_Zs, where A's blocks sit in it (offset * 2 + transposed)
	// and every camera's rows in the inner solver's permuted vector, the column passes' right-hand sides, camera parts
	// (interleaved) and column tables
	bool b_cov_sparse = false, b_cov_z_valid = false;
	CDevArray<int64_t> d_a_zent, d_cam_csn, d_cov_cols;
	CDevArray<double> d_cov_B, d_cov_X;
	std::vector<int64_t> h_cov_cols[2];        // the column tables of the last two calls (alternately)
	hipEvent_t ev_cov_cols[2] = {0, 0};        // recorded behind the uploads out of them
	int n_cov_call = 0;
	std::vector<TSchurPairRec> h_cov_pairs[2]; // the pair records of the last two calls, beside the column tables
	CDevArray<TSchurPairRec> d_cov_pairs;
	CSchurState() :p_union_fn(0), p_union_context(0), b_union_dense(false), n_union(0), b_reduced_decided(false),
		b_reduced_sparse(false), p_inner(0), n_in_blocks(0), p_sinv(0), b_sinv_tried(false) {}
	~CSchurState();
};

// the three (camera, landmark) block sizes schur_analyze admits; anything else never reaches here (schur_analyze refuses
// it with std::domain_error before a state exists, so the throw below is unreachable)
template <class F>
inline void schur_dispatch(int DC, int DP, F f)
{
	if(DC == 6 && DP == 3)
		f(std::integral_constant<int, 6>(), std::integral_constant<int, 3>());
	else if(DC == 7 && DP == 3)
		f(std::integral_constant<int, 7>(), std::integral_constant<int, 3>());
	else if(DC == 3 && DP == 2)
		f(std::integral_constant<int, 3>(), std::integral_constant<int, 2>());
	else
		throw std::logic_error("Schur path: block sizes that schur_analyze does not admit");
}

// ---- schur_setup.hip (host only) ----
// the ranks agree on the blocks of S to exchange (one-time, synchronous); how the reduced system is factored and, for the
// sparse choice, the inner solver; the tables of the sparse inverse subset (false: the dense inverse is to be used) and of
// the covariances beyond the block diagonal.  All throw.
void schur_agree_on_union(slampp_hip_solver &s, CSchurState &S);
void schur_setup_reduced(slampp_hip_solver &s, CSchurState &S);
bool schur_setup_sparse_marginals(slampp_hip_solver &s, CSchurState &S);
void schur_setup_cov_tables(slampp_hip_solver &s, CSchurState &S);

// ---- schur.hip ----
// r_c -= sum over the observations o of camera c of W_o rhs_p(o), on the camera-major lists of all observations: into p_r,
// or (p_r = 0) into the right-hand side row of the dense buffer p_S
void schur_reduced_rhs_launch(CSchurState &S, const double *rhs, double *p_S, double *p_r, hipStream_t stream);
// the reduced system of the covariances from these values (C^-1 and W of every landmark left behind): assembled into the
// inner solver's packed values and factored there / assembled into d_m_S, factored, and inverted into d_m_Z.  Throw.
void schur_marginals_sparse_factor(slampp_hip_solver &s, CSchurState &S, const double *A);
void schur_marginals_dense_inverse(slampp_hip_solver &s, CSchurState &S, const double *A);

} // namespace slampp
