// Test infrastructure (see tests/test_backward_records_host.py): the backward records of the slice tasks (TBwdHead ..,
// csrc/sparse_kernels.h), built by the panel pass of csrc/sparse_records.cpp, on the CPU.  The driver builds plan and
// records of a few graphs, fills L, inv(L_jj) and y with fixed pseudo-random numbers and runs the backward substitution
// twice in plain C++, with one column routine that follows the kernels' order of operations: once column by column from
// the Plan alone, once the way backward_slice_kernel does it -- stage by stage, the packaged tasks from their backward
// records alone, level by level, x of the task's own columns only from a per-task array, the rest tasks of the stage
// column by column.  Both results must be equal element for element.  It also checks that every internal x a level
// reads was produced by an earlier level of the same task, that the packaged tasks and the rest list of a stage are
// exactly the stage's tasks, and that every record fits the launch shape written for its stage.
#include "sparse_records.h"
#include "driver_graphs.h"
#include <cstring>
#include <map>
#include <string>

using namespace slampp;

#define REQUIRE(cond) do { if(!(cond)) { printf("%s: failed: %s (line %d)\n", name, #cond, __LINE__); return false; } } while(0)

struct TCase {
	SparseRecordOptions opt;
	Plan P;
	SparseRecords R;
	SparseLaunchLists L;
	std::set<std::string> reached;
};

// the builders in the analysis' order (as tests/sparse_records_driver.cpp runs them)
static void build_all(TCase &c)
{
	const Plan &P = c.P;
	c.L.n_bottom_stages = count_bottom_stages(P, c.opt);
	alloc_column_records(P, c.R);
	const int64_t n_upper_begin = first_upper_column(P, c.opt, c.L), n_sched = int64_t(c.R.cols.size());
	fill_column_records(P, c.R, n_upper_begin, n_sched);
	reserve_panel_packages(P, c.L, n_upper_begin, c.R);
	build_panel_packages(P, c.opt, c.R, c.L);
	fill_column_records(P, c.R, 0, n_upper_begin);
	fill_dense_top_column_records(P, c.R);
}

// one column, in the kernels' order: lane (g, q) sums its blocks g, 8 + g, .. (t ascending inside a block), the three
// butterfly steps 8, 16, 32 combine the slots, val = y - acc, x_q = sum over t >= q of inv(L_jj)[t, q] val_t (t ascending)
static void solve_column(int D, int nb, const double *const *p_blk, const double *const *p_x, const double *p_linv, const double *p_y, double *p_out)
{
	double val[8];
	for(int q = 0; q < D; ++ q) {
		double a[8];
		for(int g = 0; g < 8; ++ g) {
			double acc = 0;
			for(int kb = g; kb < nb; kb += 8) {
				for(int t = 0; t < D; ++ t)
					acc += p_blk[kb][q * D + t] * p_x[kb][t];
			}
			a[g] = acc;
		}
		for(int m = 1; m < 8; m <<= 1) {
			double r[8];
			for(int g = 0; g < 8; ++ g)
				r[g] = a[g] + a[g ^ m];
			memcpy(a, r, sizeof(a));
		}
		val[q] = p_y[q] - a[0];
	}
	for(int q = 0; q < D; ++ q) {
		double x = 0;
		for(int t = q; t < D; ++ t)
			x += p_linv[t + q * D] * val[t];
		p_out[q] = x;
	}
}

// a task column by column, last to first, from the Plan (what backward_stage_kernel does)
static void solve_task_from_plan(const Plan &P, int t, const std::vector<double> &Lv, const std::vector<double> &Linv,
	std::vector<double> &w, std::vector<double> &x_out)
{
	const int D = P.max_dim;
	std::vector<const double*> blk, xs;
	for(int64_t i = P.task_ptr[t + 1]; i > P.task_ptr[t]; -- i) {
		const int32_t j = P.task_cols[i - 1];
		blk.clear();
		xs.clear();
		for(int64_t k = P.lptr[j] + 1; k < P.lptr[j + 1]; ++ k) {
			blk.push_back(&Lv[P.loff[k]]);
			xs.push_back(&w[P.cs_new[P.lrow[k]]]);
		}
		double x[8];
		solve_column(D, int(blk.size()), blk.data(), xs.data(), &Linv[P.linv_off[j]], &w[P.cs_new[j]], x);
		for(int q = 0; q < D; ++ q)
			w[P.cs_new[j] + q] = x_out[P.cs_src[j] + q] = x[q];
	}
}

static bool check(const char *name, TCase &c)
{
	const Plan &P = c.P;
	const int D = P.max_dim, n_stages = int(P.stage_ptr.size()) - 1;
	const int64_t n_lblocks = int64_t(P.lrow.size());
	REQUIRE(P.uniform_dim && (D == 3 || D == 6 || D == 7) && P.dense_dim == 0);
	REQUIRE(!c.L.panel_ptr.empty() && int(c.L.panel_ptr.size()) == n_stages + 1 && int(c.L.panel_rest_ptr.size()) == n_stages + 1);
	REQUIRE(c.R.bwd_off.size() == c.R.panel_off.size() && int(c.L.bwd_cfg.size()) >= n_stages);
	// fixed pseudo-random numbers
	std::vector<double> Lv(size_t(P.loff[n_lblocks])), Linv(size_t(P.linv_off[P.n])), y(size_t(P.cs_new[P.n]));
	uint64_t n_state = 0x9e3779b97f4a7c15ull;
	auto Next = [&]() { n_state = n_state * 6364136223846793005ull + 1442695040888963407ull; return double(int64_t(n_state >> 11) % 2000001 - 1000000) * 1e-6; };
	for(size_t i = 0; i < Lv.size(); ++ i) Lv[i] = 0.25 * Next();
	for(size_t i = 0; i < Linv.size(); ++ i) Linv[i] = Next();
	for(size_t i = 0; i < y.size(); ++ i) y[i] = Next();
	std::vector<int32_t> col_of_cs(size_t(P.cs_new[P.n]), -1), task_of_col(size_t(P.n), -1);
	for(int32_t j = 0; j < P.n; ++ j)
		col_of_cs[size_t(P.cs_new[j])] = j;
	for(int t = 0; t < P.stage_ptr[n_stages]; ++ t) {
		for(int64_t i = P.task_ptr[t]; i < P.task_ptr[t + 1]; ++ i)
			task_of_col[P.task_cols[i]] = t;
	}
	// run A: column by column from the Plan
	std::vector<double> w_a(y), x_a(y.size(), 0.0);
	for(int s = n_stages; s > 0; -- s) {
		for(int t = P.stage_ptr[s - 1]; t < P.stage_ptr[s]; ++ t)
			solve_task_from_plan(P, t, Lv, Linv, w_a, x_a);
	}
	// run B: the packaged tasks from their backward records, the others as above
	std::vector<double> w_b(y), x_b(y.size(), 0.0);
	size_t n_records = 0;
	for(int s = n_stages; s > 0; -- s) {
		const TBwdLaunch &r_cfg = c.L.bwd_cfg[size_t(s - 1)];
		std::vector<char> task_seen(size_t(P.stage_ptr[s] - P.stage_ptr[s - 1]), 0);
		auto Mark = [&](int t) {
			if(t < P.stage_ptr[s - 1] || t >= P.stage_ptr[s] || task_seen[size_t(t - P.stage_ptr[s - 1])])
				return false;
			task_seen[size_t(t - P.stage_ptr[s - 1])] = 1;
			return true;
		};
		if(c.L.panel_ptr[s] > c.L.panel_ptr[s - 1]) {
			REQUIRE(r_cfg.n_waves >= 1 && (r_cfg.n_cols_per_wave == 1 || r_cfg.n_cols_per_wave == 2 || r_cfg.n_cols_per_wave == 4) &&
				r_cfg.n_waves * r_cfg.n_cols_per_wave <= int(PANEL_COLS) && r_cfg.n_cap_units >= 4);
			REQUIRE(backward_slice_lds_bytes(r_cfg) <= 64 * 1024);
			c.reached.insert((r_cfg.n_cols_per_wave == 1)? "one_col_per_wave" : (r_cfg.n_cols_per_wave == 2)? "two_cols_per_wave" : "four_cols_per_wave");
		}
		for(int32_t n_pkg = c.L.panel_ptr[s - 1]; n_pkg < c.L.panel_ptr[s]; ++ n_pkg, ++ n_records) {
			const int64_t n_at = c.R.bwd_off[size_t(n_pkg)] & ((int64_t(1) << BWD_OFF_BITS) - 1); // offset | units << BWD_OFF_BITS
			const int64_t n_entry_units = c.R.bwd_off[size_t(n_pkg)] >> BWD_OFF_BITS;
			REQUIRE(n_at >= 0 && n_entry_units >= 4 && size_t(n_at + n_entry_units) <= c.R.bwd_rec.size()); // (what the kernel reads stays inside)
			TBwdHead hd;
			memcpy(&hd, &c.R.bwd_rec[size_t(n_at)], sizeof(hd));
			REQUIRE(hd.n_cols >= 1 && hd.n_cols <= int(PANEL_COLS) && hd.n_levels >= 1 && hd.n_levels <= hd.n_cols && hd.n_blks >= 0);
			REQUIRE(hd.n_units == 4 + 2 * hd.n_cols + hd.n_blks && hd.n_units <= r_cfg.n_cap_units);
			REQUIRE(int64_t(hd.n_units) == n_entry_units);
			REQUIRE(hd.n_cols <= r_cfg.n_waves * r_cfg.n_cols_per_wave);
			REQUIRE(hd.lvl_ptr[0] == 0 && hd.lvl_ptr[hd.n_levels] == hd.n_cols);
			std::vector<TBwdCol> cols(size_t(hd.n_cols));
			std::vector<TBwdBlk> blks(size_t(hd.n_blks));
			memcpy(cols.data(), &c.R.bwd_rec[size_t(n_at) + 4], cols.size() * sizeof(TBwdCol));
			if(hd.n_blks)
				memcpy(blks.data(), &c.R.bwd_rec[size_t(n_at) + 4 + 2 * cols.size()], blks.size() * sizeof(TBwdBlk));
			// the record is one task of this stage, whole
			std::set<int32_t> rec_cols;
			int n_task = -1;
			for(int o = 0; o < hd.n_cols; ++ o) {
				REQUIRE(cols[o].cs_new >= 0 && size_t(cols[o].cs_new) < col_of_cs.size() && col_of_cs[size_t(cols[o].cs_new)] >= 0);
				const int32_t j = col_of_cs[size_t(cols[o].cs_new)];
				REQUIRE(cols[o].cs_src == P.cs_src[j] && cols[o].linv_off == P.linv_off[j] && cols[o].nb == int32_t(P.lptr[j + 1] - P.lptr[j]) - 1);
				REQUIRE(cols[o].blk0 >= 0 && cols[o].blk0 + cols[o].nb <= hd.n_blks);
				REQUIRE(cols[o].level >= 0 && cols[o].level < hd.n_levels && o >= hd.lvl_ptr[cols[o].level] && o < hd.lvl_ptr[cols[o].level + 1]);
				REQUIRE(rec_cols.insert(j).second && (n_task < 0 || n_task == task_of_col[j]));
				n_task = task_of_col[j];
				if(cols[o].nb > 8)
					c.reached.insert("column_over_eight_blocks");
			}
			REQUIRE(n_task >= 0 && int64_t(rec_cols.size()) == P.task_ptr[n_task + 1] - P.task_ptr[n_task] && Mark(n_task));
			if(hd.n_levels > 1)
				c.reached.insert("multi_level_task");
			if(hd.n_levels < hd.n_cols)
				c.reached.insert("level_of_several_columns");
			// level by level, last first; x of the task's own columns from s_x only
			double s_x[PANEL_COLS][8];
			int n_done_level[PANEL_COLS]; // the level that produced s_x[o], or -1
			for(int o = 0; o < int(PANEL_COLS); ++ o)
				n_done_level[o] = -1;
			for(int l = hd.n_levels - 1; l >= 0; -- l) {
				double x_level[PANEL_COLS][8];
				for(int o = hd.lvl_ptr[l]; o < hd.lvl_ptr[l + 1]; ++ o) {
					std::vector<const double*> blk, xs;
					for(int k = cols[o].blk0; k < cols[o].blk0 + cols[o].nb; ++ k) {
						REQUIRE(blks[k].loff >= 0 && blks[k].loff + D * D <= int64_t(Lv.size()));
						blk.push_back(&Lv[size_t(blks[k].loff)]);
						if(blks[k].xsrc < 0) {
							const int n_from = ~blks[k].xsrc;
							REQUIRE(n_from < hd.n_cols && n_done_level[n_from] > l); // produced by an earlier level of this task
							xs.push_back(s_x[n_from]);
							c.reached.insert("internal_x");
						} else {
							REQUIRE(size_t(blks[k].xsrc) + D <= w_b.size() && col_of_cs[size_t(blks[k].xsrc)] >= 0);
							REQUIRE(!rec_cols.count(col_of_cs[size_t(blks[k].xsrc)])); // (a row outside the task)
							xs.push_back(&w_b[size_t(blks[k].xsrc)]);
						}
					}
					solve_column(D, cols[o].nb, blk.data(), xs.data(), &Linv[size_t(cols[o].linv_off)], &w_b[size_t(cols[o].cs_new)], x_level[o]);
				}
				for(int o = hd.lvl_ptr[l]; o < hd.lvl_ptr[l + 1]; ++ o) { // (the level's columns ran side by side: published together)
					memcpy(s_x[o], x_level[o], sizeof(s_x[o]));
					n_done_level[o] = l;
					for(int q = 0; q < D; ++ q)
						w_b[size_t(cols[o].cs_new) + q] = x_b[size_t(cols[o].cs_src) + q] = x_level[o][q];
				}
			}
		}
		for(int32_t r = c.L.panel_rest_ptr[s - 1]; r < c.L.panel_rest_ptr[s]; ++ r) {
			REQUIRE(Mark(c.R.panel_rest[size_t(r)]));
			solve_task_from_plan(P, c.R.panel_rest[size_t(r)], Lv, Linv, w_b, x_b);
			c.reached.insert("rest_tasks");
		}
		const bool b_panel_stage = c.L.panel_ptr[s] > c.L.panel_ptr[s - 1] || c.L.panel_rest_ptr[s] > c.L.panel_rest_ptr[s - 1];
		for(int t = P.stage_ptr[s - 1]; t < P.stage_ptr[s]; ++ t) {
			REQUIRE(bool(task_seen[size_t(t - P.stage_ptr[s - 1])]) == b_panel_stage); // the two lists together: exactly the stage's tasks
			if(!b_panel_stage)
				solve_task_from_plan(P, t, Lv, Linv, w_b, x_b);
		}
		if(b_panel_stage)
			c.reached.insert("slice_stages");
	}
	REQUIRE(n_records == c.R.bwd_off.size());
	REQUIRE(w_a.size() == w_b.size() && memcmp(w_a.data(), w_b.data(), w_a.size() * sizeof(double)) == 0);
	REQUIRE(memcmp(x_a.data(), x_b.data(), x_a.size() * sizeof(double)) == 0);
	bool b_moved = false;
	for(size_t i = 0; i < y.size(); ++ i)
		b_moved = b_moved || w_a[i] != y[i];
	REQUIRE(b_moved);
	return true;
}

static bool run(const char *name, int n, const CEdgeList &edges, int n_dim, const SparseRecordOptions &rec_opt)
{
	TCase c;
	c.opt = rec_opt;
	PlanOptions plan_opt; // subtree_size 4, leaf_size 1, dense_top_nb 0 (tests/variant_util.py: PLAN_OPTIONS)
	plan_opt.subtree_size = 4;
	plan_opt.leaf_size = 1;
	plan_opt.dense_top_nb = 0;
	plan_opt.task_wide_min = std::max(rec_opt.n_wide_min_tasks, 1); // (what the analysis sets before it plans: the panel kernel's capacities)
	plan_opt.task_max_cols = int(PANEL_COLS);
	plan_opt.task_max_blocks = panel_slot_cap(n_dim);
	if(!plan_of_graph(name, n, edges, std::vector<int>(1, n_dim), plan_opt, c.P))
		return false;
	build_all(c);
	if(!check(name, c))
		return false;
	printf("%s: columns %d stages %d records %zu reached", name, c.P.n, int(c.P.stage_ptr.size()) - 1, c.R.bwd_off.size());
	for(std::set<std::string>::const_iterator p = c.reached.begin(); p != c.reached.end(); ++ p)
		printf(" %s", p->c_str());
	printf(" ok\n");
	return true;
}

int main()
{
	setenv("SLAMPP_HIP_DEV", "1", 1); // (the development knobs below are read only with it: plan.h)
	dev_knobs_refresh();
	std::mt19937 rng(7);
	bool b_ok = true;
	const SparseRecordOptions t_default = {-1, 1, -1, 32, 1, 8192, true, false};
	const int sizes[] = {40, 300, 612}, dims[] = {3, 6, 7};
	for(int i = 0; i < 3; ++ i) {
		const CEdgeList chain = chain_with_closures(sizes[i], rng);
		for(int d = 0; d < 3; ++ d)
			b_ok = run(("chain" + std::to_string(dims[d]) + "-" + std::to_string(sizes[i])).c_str(), sizes[i], chain, dims[d], t_default) && b_ok;
		if(sizes[i] == 612) { // the launch shapes of crowded stages: two and four columns per wave
			SparseRecordOptions t_opt = t_default;
			t_opt.n_wide_min_tasks = 8;
			setenv("SLAMPP_HIP_DEV_PANEL_W4_MIN", "0", 1);
			b_ok = run("chain6-612-four-waves", 612, chain, 6, t_opt) && b_ok;
			setenv("SLAMPP_HIP_DEV_PANEL_W2_MIN", "0", 1);
			b_ok = run("chain7-612-two-waves", 612, chain, 7, t_opt) && b_ok;
			unsetenv("SLAMPP_HIP_DEV_PANEL_W4_MIN");
			unsetenv("SLAMPP_HIP_DEV_PANEL_W2_MIN");
		}
	}
	{ // a hub (tests/variant_util.py: hub_chain): a chain plus one vertex joined to 60 poses and a banded stretch -- a column
	  // with more than nine blocks, a task over the panel capacities
		const int n = 300;
		CEdgeList e = chain_with_closures(n, rng);
		for(int i = 10; i < 70; ++ i)
			e.push_back(std::make_pair(i, n));
		for(int i = 180; i < 260; ++ i) {
			e.push_back(std::make_pair(i, i + 2));
			e.push_back(std::make_pair(i, i + 3));
		}
		for(int d = 0; d < 3; ++ d)
			b_ok = run(("hub" + std::to_string(dims[d])).c_str(), n + 1, e, dims[d], t_default) && b_ok;
		// ... and with a clique of 110 hanging off pose 150, whose first columns have more blocks than an image has slots (as
		// tests/sparse_records_driver.cpp has it): tasks left to the column kernel beside packaged ones
		const int n_clique = 110;
		for(int i = 0; i < n_clique; ++ i) {
			e.push_back(std::make_pair(150, n + 1 + i));
			for(int k = 0; k < i; ++ k)
				e.push_back(std::make_pair(n + 1 + k, n + 1 + i));
		}
		SparseRecordOptions t_opt = t_default;
		t_opt.n_wide_min_tasks = 8;
		for(int d = 0; d < 3; ++ d)
			b_ok = run(("hub-clique" + std::to_string(dims[d])).c_str(), n + 1 + n_clique, e, dims[d], t_opt) && b_ok;
	}
	return b_ok? 0 : 1;
}
