// covariance.h -- covariances beyond the block diagonal (covariance.hip): Lambda^-1 on Lambda's own block pattern, and
// whole block columns of Lambda^-1 by multi-right-hand-side triangular solves with the factor in place
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct slampp_hip_solver;

namespace slampp {

struct CCovariance;
struct PairPlan;

// scalar columns of one pass of slampp_hip_marginal_columns: the workspace is n_scalars x COV_K_PASS doubles.  48 = eight
// 6 x 6 block columns (or six 8 x 8 ones) in one pass; a lane of a wave per right-hand side, 48 of its 64 lanes busy
enum { COV_K_PASS = 48 };

void covariance_destroy(CCovariance *p);
size_t covariance_bytes(const CCovariance *p);

// Lambda^-1 at every stored (upper) block of Lambda, in the layout of Lambda's packed values, from the sparse inverse
// subset Z (laid out like L) and -- with a dense top -- the dense inverse of the top's Schur complement Zd (lower
// triangle and diagonal tiles valid, leading dimension s.n_dense_pad).  Builds its gather records at the first call
// (Lambda's pattern lies inside the factor's: checked there, on the host).  Throws.
void covariance_pattern_enqueue(slampp_hip_solver &s, double *p_out_dev);

// block columns p_bcols[0 .. n_cols) (caller's order, distinct, in range: checked by the caller) of Lambda^-1 from the factor
// in place (d_L, d_Linv of every column, the dense top's factor and inverted diagonal tiles): p_out_dev is n_scalars x k,
// column-major, rows in the caller's scalar order, k = the sum of the columns' dimensions.  Throws.
void covariance_columns_enqueue(slampp_hip_solver &s, int n_cols, const int64_t *p_bcols, double *p_out_dev);

// blocks (p_brows[k], p_bcols[k]) of Lambda^-1, k = 0 .. n_pairs (caller's block columns, in range: checked by the caller; any
// order, repeats allowed), from the factor in place: Y_r^T Y_c from the pruned forward substitution alone, summed over the
// rows the two elimination-tree paths share (pair_plan.h) in a fixed order.  p_out_dev: the d_r x d_c blocks, column-major,
// one after the other in the listed order.  Throws.
void covariance_pairs_enqueue(slampp_hip_solver &s, int64_t n_pairs, const int64_t *p_brows, const int64_t *p_bcols, double *p_out_dev);

// The same for pairs of columns whose right-hand sides are given whole, in two steps.  covariance_pair_sets_plan: pair k is
// (p_set_r[k], p_set_c[k]) of n_sets column sets, set i nonzero on the rows of the block columns p_set_src[p_set_ptr[i] ..
// p_set_ptr[i + 1]) (new order) only and p_set_width[i] scalar right-hand sides wide (plan_pair_sets, pair_plan.h); plans the
// passes, lists their forward substitutions and uploads every list of the call, enqueues no kernel.  The plan it returns
// (valid until the next covariance call on s) says which sets each pass holds and in which lanes.
// covariance_pair_sets_pass: pass n_pass of that plan, its right-hand sides in p_rhs_dev (the factor's permuted row order,
// interleaved: row * kp + lane): the pruned forward substitution and the Gram products into p_out_dev at the offsets the
// plan gives.  Throw.
const PairPlan &covariance_pair_sets_plan(slampp_hip_solver &s, int64_t n_pairs, const int32_t *p_set_r, const int32_t *p_set_c,
	int32_t n_sets, const int64_t *p_set_ptr, const int32_t *p_set_src, const int32_t *p_set_width);
void covariance_pair_sets_pass(slampp_hip_solver &s, size_t n_pass, const double *p_rhs_dev, double *p_out_dev);

// one pass of kp <= COV_K_PASS right-hand sides given whole: p_rhs_dev is n_scalars x kp in the factor's permuted row order,
// interleaved (row * kp + column), nonzero on the rows of the block columns p_src_bcols[0 .. n_src) only (the pruned forward
// substitution starts from their elimination-tree paths).  The solution goes to p_out_dev + n_col0 * n_ld_out, column-major,
// rows in the caller's scalar order.  Throws.
void covariance_columns_rhs_enqueue(slampp_hip_solver &s, int n_src, const int64_t *p_src_bcols, int kp, const double *p_rhs_dev,
	double *p_out_dev, int64_t n_ld_out, int64_t n_col0);

// n_columns right-hand sides given whole, solved in place from the factor in place (slampp_hip_solve_columns): column c is
// the n_scalars doubles at p_rhs_dev + c * n_ld, rows in the caller's scalar order.  Unpruned k-column substitutions over
// the static device plan, in passes of COV_K_PASS columns through the interleaved workspace; the dense top by the k-column
// tile solves above.  solve_columns_applies: the plan has kernels for it (no block column wider than 8, which the analysis
// would have cut into pieces); the caller solves column by column otherwise.  Enqueue-only but for the first call after an
// analysis, which builds the dense-top columns' row lists on the host.  Throws.
bool solve_columns_applies(const slampp_hip_solver &s);
void solve_columns_enqueue(slampp_hip_solver &s, double *p_rhs_dev, int64_t n_ld, int n_columns);

// One of the two substitutions alone, on the same columns (slampp_hip_solve_half_columns; needs solve_columns_applies).
// Forward: column c holds b in the caller's scalar order on entry and y = L^-1 P b in the factor's order (Plan::cs_new) on
// return; backward: y in the factor's order on entry, x = P^T L^-T y in the caller's order on return.  The launches of
// solve_columns_enqueue, in its order, cut in two: the forward half ends with y copied out of the interleaved workspace (the
// dense top's rows out of the tile solves' array), the backward half begins with y copied in.  The workspace stays in
// between because the forward kernels read b at cs_src while other tasks already write y at cs_new.  One after the other
// they give solve_columns_enqueue's bits.  Throws.
void solve_half_columns_enqueue(slampp_hip_solver &s, bool b_backward, double *p_inout_dev, int64_t n_ld, int n_columns);

} // namespace slampp
