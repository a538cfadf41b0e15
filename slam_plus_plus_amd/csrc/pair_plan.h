// pair_plan.h -- host planning of covariance blocks at arbitrary block pairs (slampp_hip_marginal_blocks).  With
// Lambda = P^T L L^T P, block (r, c) of Lambda^-1 is Y_r^T Y_c, Y_j = L^-1 P E_j, and Y_j is nonzero only on the path of j
// to the root of the elimination tree: the product runs over the rows the two paths share, path(lca(r, c) -> root), and
// over the dense top where both paths reach it.  The pairs are grouped into passes of the pruned forward substitution
// (covariance.hip); this file says which columns a pass holds, in which lanes, and which rows every pair sums over.
// A column may also be a set of source block columns with a scalar width (plan_pair_sets): Y = L^-1 P B for a right-hand side
// B that is nonzero on the sources' rows only -- the camera and landmark columns of a BA system over its reduced camera
// system (schur_covariance.hip).  Such a Y is nonzero on its reach, the union of the sources' paths to the root, and a pair
// sums over the rows both reaches hold.
// Depends on plan.h only, no device calls: compiled on its own under the sanitizers (tests/pair_plan_driver.cpp).
#pragma once
#include "plan.h"

namespace slampp {

struct TPairRow { // 8 B: one block-eliminated column on a pair's shared path
	int32_t cs;  // first permuted scalar row (Plan::cs_new)
	int32_t dim;
};

struct TPairRec { // 40 B: one pair
	int64_t out;      // offset of its d_r x d_c block (column-major) in the output: the caller's position
	int64_t row0;     // its rows: TPairRow[row0 .. row0 + n_rows), in schedule order
	int32_t n_rows;
	int32_t lane_r, lane_c; // first right-hand side of block column r / c in its pass
	int32_t dr, dc;
	int32_t dense;    // 1: the dense top's rows follow (both paths reach the top)
};

struct TPairPass {
	int32_t kp = 0;                 // scalar right-hand sides in use (<= the limit given to plan_pairs)
	std::vector<int32_t> cols;      // distinct block columns (new order; plan_pair_sets: column sets), in order of first appearance
	std::vector<int32_t> lanes;     // first right-hand side of each
	int64_t pair0 = 0, pair1 = 0;   // its pairs: PairPlan::pairs[pair0 .. pair1)
	bool b_dense = false;           // one of its pairs sums over the dense top
	std::vector<int32_t> srcs;      // plan_pair_sets only: the distinct source block columns (new order) of its sets
};

struct PairPlan {
	std::vector<TPairPass> passes;
	std::vector<TPairRec> pairs;    // in the caller's order (passes take consecutive runs of it)
	std::vector<TPairRow> rows;
	int64_t n_out = 0;              // doubles of the output
};

// schedule index of every column (new order) of a plan, -1 for the columns of the dense top
std::vector<int32_t> pair_sched_pos(const Plan &plan);

// Plans n_pairs pairs of block columns (caller's order, in range: checked by the caller; any order, repeats allowed).
// Greedy grouping: pairs are taken in the given order until the distinct columns of the next one would not fit into
// n_k_pass scalar right-hand sides.  sched_pos: pair_sched_pos(plan).  Throws std::invalid_argument if a single pair
// does not fit a pass.
void plan_pairs(const Plan &plan, const std::vector<int32_t> &sched_pos, int64_t n_pairs, const int64_t *p_brows,
	const int64_t *p_bcols, int n_k_pass, PairPlan &r_out);

// The same for pairs (p_set_r[k], p_set_c[k]) of column sets: set i has the source block columns
// p_set_src[p_set_ptr[i] .. p_set_ptr[i + 1]) (new order, at least one) and p_set_width[i] scalar right-hand sides.  A pair's
// rows are the intersection of the two sets' reaches (ancestor-closed, as each reach is), in schedule order; it sums over
// the dense top when both reaches enter it.  TPairPass::cols holds set indices, TPairPass::srcs the sources the pruned
// forward substitution of the pass starts from.  Sets of one source each, as wide as that block column, give the records
// of plan_pairs.  Throws std::invalid_argument for a set index out of range or a pair that does not fit a pass.
void plan_pair_sets(const Plan &plan, const std::vector<int32_t> &sched_pos, int64_t n_pairs, const int32_t *p_set_r,
	const int32_t *p_set_c, int32_t n_sets, const int64_t *p_set_ptr, const int32_t *p_set_src, const int32_t *p_set_width,
	int n_k_pass, PairPlan &r_out);

} // namespace slampp
