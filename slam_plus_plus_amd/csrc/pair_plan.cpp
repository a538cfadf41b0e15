// pair_plan.cpp -- see pair_plan.h
#include "pair_plan.h"

#include <algorithm>
#include <stdexcept>

namespace slampp {

std::vector<int32_t> pair_sched_pos(const Plan &plan)
{
	std::vector<int32_t> pos(size_t(plan.n), -1);
	for(size_t sc = 0; sc < plan.task_cols.size(); ++ sc)
		pos[size_t(plan.task_cols[sc])] = int32_t(sc);
	return pos;
}

// the pass of pair k: both columns (ids id_r, id_c, d_r and d_c scalar right-hand sides wide) in the current pass if they
// fit, else in a new one; their lanes into r_rec
static void place_pair(std::vector<TPairPass> &r_passes, int64_t k, int32_t id_r, int32_t id_c, int n_k_pass, TPairRec &r_rec)
{
	for(int n_try = 0;; ++ n_try) {
		if(r_passes.empty() || n_try) {
			r_passes.push_back(TPairPass());
			r_passes.back().pair0 = r_passes.back().pair1 = k;
		}
		TPairPass &pass = r_passes.back();
		const size_t n_none = pass.cols.size(); // (positions, not iterators: the columns are appended to below)
		const size_t n_at_r = size_t(std::find(pass.cols.begin(), pass.cols.end(), id_r) - pass.cols.begin()),
			n_at_c = (id_c == id_r)? n_at_r : size_t(std::find(pass.cols.begin(), pass.cols.end(), id_c) - pass.cols.begin());
		const int n_more = ((n_at_r == n_none)? r_rec.dr : 0) + ((n_at_c == n_none && id_c != id_r)? r_rec.dc : 0);
		if(pass.kp + n_more > n_k_pass) {
			if(n_try || pass.cols.empty())
				throw std::invalid_argument("marginal_blocks: a pair of block columns does not fit one pass");
			continue;
		}
		if(n_at_r == n_none) {
			pass.cols.push_back(id_r);
			pass.lanes.push_back(pass.kp);
			pass.kp += r_rec.dr;
		}
		r_rec.lane_r = pass.lanes[n_at_r];
		if(n_at_c == n_none && id_c != id_r) {
			pass.cols.push_back(id_c);
			pass.lanes.push_back(pass.kp);
			pass.kp += r_rec.dc;
		}
		r_rec.lane_c = pass.lanes[(id_c == id_r)? n_at_r : (n_at_c == n_none)? pass.cols.size() - 1 : n_at_c];
		return;
	}
}

// the rows of a pair (the block-eliminated columns in r_shared, any order) and its place in the output, into r_rec and r_out
static void finish_pair(const Plan &plan, const std::vector<int32_t> &sched_pos, std::vector<int32_t> &r_shared, bool b_dense,
	int64_t k, TPairRec &r_rec, PairPlan &r_out)
{
	std::sort(r_shared.begin(), r_shared.end(), [&](int32_t a, int32_t b) { return sched_pos[size_t(a)] < sched_pos[size_t(b)]; });
	r_rec.row0 = int64_t(r_out.rows.size());
	r_rec.n_rows = int32_t(r_shared.size());
	for(size_t q = 0; q < r_shared.size(); ++ q) {
		TPairRow row = {int32_t(plan.cs_new[size_t(r_shared[q])]), plan.dim[size_t(r_shared[q])]};
		r_out.rows.push_back(row);
	}
	r_rec.dense = b_dense? 1 : 0;
	r_rec.out = r_out.n_out;
	r_out.n_out += int64_t(r_rec.dr) * r_rec.dc;
	r_out.pairs.push_back(r_rec);
	TPairPass &pass = r_out.passes.back();
	pass.pair1 = k + 1;
	pass.b_dense = pass.b_dense || b_dense;
}

static void clear_plan(PairPlan &r_out, int64_t n_pairs)
{
	r_out.passes.clear();
	r_out.pairs.clear();
	r_out.rows.clear();
	r_out.n_out = 0;
	r_out.pairs.reserve(size_t(std::max<int64_t>(n_pairs, 0)));
}

void plan_pairs(const Plan &plan, const std::vector<int32_t> &sched_pos, int64_t n_pairs, const int64_t *p_brows,
	const int64_t *p_bcols, int n_k_pass, PairPlan &r_out)
{
	clear_plan(r_out, n_pairs);
	std::vector<int64_t> mark(size_t(plan.n), -1); // mark[x] = k: x is on the path of pair k's row column
	std::vector<int32_t> shared;
	for(int64_t k = 0; k < n_pairs; ++ k) {
		const int32_t jr = plan.pinv[size_t(p_brows[k])], jc = plan.pinv[size_t(p_bcols[k])];
		TPairRec rec;
		rec.dr = plan.dim[size_t(jr)];
		rec.dc = plan.dim[size_t(jc)];
		place_pair(r_out.passes, k, jr, jc, n_k_pass, rec);
		// the rows: the paths of the two columns meet at their lowest common ancestor and stay together to the root
		bool b_top_r = false, b_top_c = false;
		for(int32_t x = jr; x >= 0; x = plan.parent[size_t(x)]) {
			mark[size_t(x)] = k;
			b_top_r = b_top_r || sched_pos[size_t(x)] < 0;
		}
		shared.clear();
		bool b_met = false;
		for(int32_t x = jc; x >= 0; x = plan.parent[size_t(x)]) {
			b_met = b_met || mark[size_t(x)] == k;
			b_top_c = b_top_c || sched_pos[size_t(x)] < 0;
			if(b_met && sched_pos[size_t(x)] >= 0)
				shared.push_back(x);
		}
		finish_pair(plan, sched_pos, shared, b_top_r && b_top_c, k, rec, r_out);
	}
}

void plan_pair_sets(const Plan &plan, const std::vector<int32_t> &sched_pos, int64_t n_pairs, const int32_t *p_set_r,
	const int32_t *p_set_c, int32_t n_sets, const int64_t *p_set_ptr, const int32_t *p_set_src, const int32_t *p_set_width,
	int n_k_pass, PairPlan &r_out)
{
	clear_plan(r_out, n_pairs);
	// mark_r[x] = k: x is in the reach of pair k's row set; mark_c[x] = k: the walk from its column set has passed x
	std::vector<int64_t> mark_r(size_t(plan.n), -1), mark_c(size_t(plan.n), -1);
	std::vector<int64_t> src_pass(size_t(plan.n), -1); // src_pass[j] = p: j is among the sources of pass p
	std::vector<int32_t> shared;
	for(int64_t k = 0; k < n_pairs; ++ k) {
		const int32_t sr = p_set_r[k], sc = p_set_c[k];
		if(sr < 0 || sr >= n_sets || sc < 0 || sc >= n_sets)
			throw std::invalid_argument("marginal_blocks: a pair names a column set that was not given");
		TPairRec rec;
		rec.dr = p_set_width[sr];
		rec.dc = p_set_width[sc];
		place_pair(r_out.passes, k, sr, sc, n_k_pass, rec);
		TPairPass &pass = r_out.passes.back();
		const int64_t n_pass = int64_t(r_out.passes.size()) - 1;
		bool b_top_r = false, b_top_c = false;
		for(int64_t i = p_set_ptr[sr]; i < p_set_ptr[sr + 1]; ++ i) {
			const int32_t j = p_set_src[i];
			if(src_pass[size_t(j)] != n_pass) {
				src_pass[size_t(j)] = n_pass;
				pass.srcs.push_back(j);
			}
			for(int32_t x = j; x >= 0 && mark_r[size_t(x)] != k; x = plan.parent[size_t(x)]) {
				mark_r[size_t(x)] = k; // (an ancestor met before has its whole path marked)
				b_top_r = b_top_r || sched_pos[size_t(x)] < 0;
			}
		}
		shared.clear();
		for(int64_t i = p_set_ptr[sc]; i < p_set_ptr[sc + 1]; ++ i) {
			const int32_t j = p_set_src[i];
			if(src_pass[size_t(j)] != n_pass) {
				src_pass[size_t(j)] = n_pass;
				pass.srcs.push_back(j);
			}
			for(int32_t x = j; x >= 0 && mark_c[size_t(x)] != k; x = plan.parent[size_t(x)]) {
				mark_c[size_t(x)] = k;
				b_top_c = b_top_c || sched_pos[size_t(x)] < 0;
				if(mark_r[size_t(x)] == k && sched_pos[size_t(x)] >= 0)
					shared.push_back(x); // (every column of the second reach is passed once)
			}
		}
		finish_pair(plan, sched_pos, shared, b_top_r && b_top_c, k, rec, r_out);
	}
}

} // namespace slampp
