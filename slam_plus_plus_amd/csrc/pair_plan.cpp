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

void plan_pairs(const Plan &plan, const std::vector<int32_t> &sched_pos, int64_t n_pairs, const int64_t *p_brows,
	const int64_t *p_bcols, int n_k_pass, PairPlan &r_out)
{
	r_out.passes.clear();
	r_out.pairs.clear();
	r_out.rows.clear();
	r_out.n_out = 0;
	r_out.pairs.reserve(size_t(std::max<int64_t>(n_pairs, 0)));
	std::vector<int64_t> mark(size_t(plan.n), -1); // mark[x] = k: x is on the path of pair k's row column
	std::vector<int32_t> shared;
	for(int64_t k = 0; k < n_pairs; ++ k) {
		const int32_t jr = plan.pinv[size_t(p_brows[k])], jc = plan.pinv[size_t(p_bcols[k])];
		TPairRec rec;
		rec.dr = plan.dim[size_t(jr)];
		rec.dc = plan.dim[size_t(jc)];
		// the pass: both columns in the current one if they fit, else a new one
		for(int n_try = 0;; ++ n_try) {
			if(r_out.passes.empty() || n_try) {
				r_out.passes.push_back(TPairPass());
				r_out.passes.back().pair0 = r_out.passes.back().pair1 = k;
			}
			TPairPass &pass = r_out.passes.back();
			const size_t n_none = pass.cols.size(); // (positions, not iterators: the columns are appended to below)
			const size_t n_at_r = size_t(std::find(pass.cols.begin(), pass.cols.end(), jr) - pass.cols.begin()),
				n_at_c = (jc == jr)? n_at_r : size_t(std::find(pass.cols.begin(), pass.cols.end(), jc) - pass.cols.begin());
			const int n_more = ((n_at_r == n_none)? rec.dr : 0) + ((n_at_c == n_none && jc != jr)? rec.dc : 0);
			if(pass.kp + n_more > n_k_pass) {
				if(n_try || pass.cols.empty())
					throw std::invalid_argument("marginal_blocks: a pair of block columns does not fit one pass");
				continue;
			}
			if(n_at_r == n_none) {
				pass.cols.push_back(jr);
				pass.lanes.push_back(pass.kp);
				pass.kp += rec.dr;
			}
			rec.lane_r = pass.lanes[n_at_r];
			if(n_at_c == n_none && jc != jr) {
				pass.cols.push_back(jc);
				pass.lanes.push_back(pass.kp);
				pass.kp += rec.dc;
			}
			rec.lane_c = pass.lanes[(jc == jr)? n_at_r : (n_at_c == n_none)? pass.cols.size() - 1 : n_at_c];
			break;
		}
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
		std::sort(shared.begin(), shared.end(), [&](int32_t a, int32_t b) { return sched_pos[size_t(a)] < sched_pos[size_t(b)]; });
		rec.row0 = int64_t(r_out.rows.size());
		rec.n_rows = int32_t(shared.size());
		for(size_t q = 0; q < shared.size(); ++ q) {
			TPairRow row = {int32_t(plan.cs_new[size_t(shared[q])]), plan.dim[size_t(shared[q])]};
			r_out.rows.push_back(row);
		}
		rec.dense = (b_top_r && b_top_c)? 1 : 0;
		rec.out = r_out.n_out;
		r_out.n_out += int64_t(rec.dr) * rec.dc;
		r_out.pairs.push_back(rec);
		TPairPass &pass = r_out.passes.back();
		pass.pair1 = k + 1;
		pass.b_dense = pass.b_dense || rec.dense != 0;
	}
}

} // namespace slampp
