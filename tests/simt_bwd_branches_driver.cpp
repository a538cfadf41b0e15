// Test infrastructure (see tests/test_simt_bwd_branches_host.py): the workgroup records of the two-wave leaf backward form
// (csrc/sparse_kernels.h: TSimtBwdBranchLaunch; csrc/sparse_records.cpp: Build_Simt_Bwd_Branches()) on the CPU.  The driver
// builds plan and lane-per-task tables of a few graphs with every two-bin shape split, and checks from the records alone: of
// every split task that each of its columns lies in exactly one segment, that the places the segments' columns carry are a
// permutation of the task's columns (each column its own place), that every row of a bin's column that lies inside the task
// is a column of the same bin or a join, and that the three segments hold the same task in the same lane; of every segment
// that its table and the places of its columns fit the LDS regions of the stage; of every stage that its records cover every
// chunk exactly once, in the order of the factor form's records.  It runs the backward substitution twice in plain C++ with
// one column routine -- task by task from the Plan with x in the workspace, and record by record (joins, bin 0, bin 1) from the
// segments' programs and tables with x of the task's own columns in an array indexed by place, as the kernel keeps it in LDS --
// and requires the solutions equal element for element.  Last, it builds the tables once more without any records and
// requires the chunk, program and table arrays the one-wave forms read to be the same bytes.
#include "sparse_records.h"
#include "driver_graphs.h"
#include <cmath>
#include <cstring>
#include <map>
#include <string>

using namespace slampp;

#define REQUIRE(cond) do { if(!(cond)) { printf("%s: failed: %s (line %d)\n", name, #cond, __LINE__); return false; } } while(0)

// one column of the substitution as a lane sees it: offsets, and per block below the diagonal where x of its row comes from
struct TBwdColumn {
	int64_t l_base, cs_new, cs_src;
	int n_place;                       // where x of this column goes among the task's own (-1: run from the Plan, everything through w)
	std::vector<int64_t> x_off;        // per block below the diagonal: the scalar offset of its row in the workspace
	std::vector<int32_t> n_local;      // and which of the task's columns the row is, or -1
};

// x_j = L_jj^-T (y_j - sum_i L(i,j)^T x_i), in the kernels' order of operations (csrc/simt_kernel.hip: bwd_ahead_solve())
static void backward_column(int D, const TBwdColumn &c, const std::vector<double> &L, std::vector<double> &w, std::vector<double> &x_out,
	std::vector<double> &x_own /* [place][D] */)
{
	double acc[8], x[8];
	for(int q = 0; q < D; ++ q)
		acc[q] = w[size_t(c.cs_new + q)];
	for(size_t kb = 0; kb < c.x_off.size(); ++ kb) {
		const double *blk = &L[size_t(c.l_base + int64_t(kb + 1) * D * D)];
		const double *xi = (c.n_place >= 0 && c.n_local[kb] >= 0)? &x_own[size_t(c.n_local[kb]) * size_t(D)] : &w[size_t(c.x_off[kb])];
		for(int q = 0; q < D; ++ q) {
			for(int r = 0; r < D; ++ r)
				acc[q] -= blk[r + q * D] * xi[r];
		}
	}
	const double *a = &L[size_t(c.l_base)];
	for(int q = D - 1; q >= 0; -- q) {
		double sum = acc[q];
		for(int r = q + 1; r < D; ++ r)
			sum -= a[r + q * D] * x[r];
		x[q] = sum * (1.0 / a[q + q * D]);
	}
	for(int q = 0; q < D; ++ q) {
		if(c.n_place >= 0)
			x_own[size_t(c.n_place) * size_t(D) + size_t(q)] = x[q];
		w[size_t(c.cs_new + q)] = x[q];
		x_out[size_t(c.cs_src + q)] = x[q];
	}
}

// the columns of one lane of a backward segment, first to last, from its program and table alone; false: malformed
static bool columns_from_segment(const SparseRecords &R, const TSimtChunk &ch, int W, int n_lane, std::vector<TBwdColumn> &cols)
{
	cols.clear();
	if(ch.prog_off < 0 || size_t(ch.prog_off) + 2 > R.simt_bwd_prog.size())
		return false;
	const int32_t *P = &R.simt_bwd_prog[size_t(ch.prog_off)];
	const int n_cols = P[0], n_below = P[1];
	if(n_cols < 1 || n_below < 0 || size_t(ch.prog_off) + 2 + 2 * size_t(n_cols) + size_t(n_below) > R.simt_bwd_prog.size())
		return false;
	if(ch.tab_off < 0 || size_t(ch.tab_off) + size_t(3 * n_cols + n_below) * size_t(W) > R.simt_bwd_tab.size())
		return false;
	const int64_t *T = &R.simt_bwd_tab[size_t(ch.tab_off)] + n_lane;
	const int32_t *p_nb = P + 2, *p_local = p_nb + n_cols, *p_place = p_local + n_below;
	int n_blk = 0;
	for(int ci = 0; ci < n_cols; ++ ci) {
		TBwdColumn c;
		c.l_base = T[W * (3 * ci)]; c.cs_new = T[W * (3 * ci + 1)]; c.cs_src = T[W * (3 * ci + 2)];
		c.n_place = p_place[ci];
		if(p_nb[ci] < 1 || n_blk + p_nb[ci] - 1 > n_below || c.n_place < 0)
			return false;
		for(int kb = 1; kb < p_nb[ci]; ++ kb, ++ n_blk) {
			c.x_off.push_back(T[W * (3 * n_cols + n_blk)]);
			c.n_local.push_back(p_local[n_blk]);
		}
		cols.push_back(c);
	}
	return n_blk == n_below;
}

struct TCase {
	SparseRecordOptions opt;
	Plan P;
	SparseRecords R;
	SparseLaunchLists L;
	std::set<std::string> reached;
};

static bool check(const char *name, TCase &c)
{
	const Plan &P = c.P;
	const SparseRecords &R = c.R;
	const int D = P.max_dim, W = c.opt.n_simt_width;
	REQUIRE(P.uniform_dim && D == 6 && P.dense_dim == 0);
	REQUIRE(!c.L.simt_chunk_ptr.empty() && c.L.simt_br.size() + 1 == c.L.simt_chunk_ptr.size());
	std::vector<int32_t> col_of_cs(size_t(P.cs_new[P.n]) + 1, -1), task_of_col(size_t(P.n), -1);
	for(int32_t j = 0; j < P.n; ++ j)
		col_of_cs[size_t(P.cs_new[j])] = j;
	const int n_stages = int(P.stage_ptr.size()) - 1;
	for(int t = 0; t < P.stage_ptr[n_stages]; ++ t) {
		for(int64_t i = P.task_ptr[t]; i < P.task_ptr[t + 1]; ++ i)
			task_of_col[size_t(P.task_cols[size_t(i)])] = t;
	}
	// fixed pseudo-random numbers: a factor with heavy diagonals, y in the workspace
	std::vector<double> L(size_t(P.loff[P.lrow.size()])), w0(size_t(P.cs_new[P.n])), x0(size_t(P.cs_new[P.n]), -7.0);
	uint64_t n_state = 0x9e3779b97f4a7c15ull;
	auto Next = [&]() { n_state = n_state * 6364136223846793005ull + 1442695040888963407ull; return double(int64_t(n_state >> 11) % 2000001 - 1000000) * 1e-6; };
	for(size_t i = 0; i < L.size(); ++ i) L[i] = 0.3 * Next();
	for(size_t i = 0; i < w0.size(); ++ i) w0[i] = Next();
	for(int32_t j = 0; j < P.n; ++ j) {
		for(int q = 0; q < D; ++ q)
			L[size_t(P.loff[size_t(P.lptr[j])] + q + q * D)] += 3.0;
	}
	std::vector<double> w_plan(w0), w_rec(w0), x_plan(x0), x_rec(x0), x_own;
	std::vector<TBwdColumn> cols;
	for(size_t s = c.L.simt_chunk_ptr.size() - 1; s -- > 0;) { // (stages last to first, as the substitution runs them; the stages above keep y: their x is not needed for the comparison)
		const TSimtBranchStage &br = c.L.simt_br[s];
		REQUIRE(br.n_groups > 0 && br.n_bwd_groups == br.n_groups && size_t(br.n_bwd_first + br.n_bwd_groups) <= R.simt_bwd_br_groups.size());
		REQUIRE(br.n_bwd_lds_bytes > 0 && br.n_bwd_lds_bytes <= 64 * 1024 && br.n_bwd_lds_bytes == (3 * br.n_bwd_tab_region + 2 * br.n_bwd_x_region) * 8);
		const int32_t n_chunk0 = c.L.simt_chunk_ptr[s], n_chunk1 = c.L.simt_chunk_ptr[s + 1];
		// run A: the stage's lane-per-task tasks one by one from the Plan, columns last to first
		std::map<int32_t, int32_t> chunk_of_first_task;
		for(int32_t n_chunk = n_chunk0; n_chunk < n_chunk1; ++ n_chunk) {
			const TSimtChunk &ch = R.simt_bwd_chunks[size_t(n_chunk)];
			REQUIRE(ch.n_tasks >= 1 && ch.n_tasks <= W);
			const int64_t *T = &R.simt_bwd_tab[size_t(ch.tab_off)];
			for(int n_lane = 0; n_lane < ch.n_tasks; ++ n_lane) {
				const int32_t t = task_of_col[size_t(col_of_cs[size_t(T[W * 1 + n_lane])])];
				if(n_lane == 0)
					chunk_of_first_task[t] = n_chunk;
				for(int64_t i = P.task_ptr[t + 1]; i -- > P.task_ptr[t];) {
					const int32_t j = P.task_cols[size_t(i)];
					TBwdColumn t_col;
					t_col.l_base = P.loff[size_t(P.lptr[j])]; t_col.cs_new = P.cs_new[j]; t_col.cs_src = P.cs_src[j]; t_col.n_place = -1;
					for(int64_t k = P.lptr[j] + 1; k < P.lptr[j + 1]; ++ k) {
						t_col.x_off.push_back(P.cs_new[P.lrow[size_t(k)]]);
						t_col.n_local.push_back(-1);
					}
					backward_column(D, t_col, L, w_plan, x_plan, x_own);
				}
			}
		}
		// run B: record by record: the joins, then the bins
		std::vector<char> chunk_seen(size_t(n_chunk1 - n_chunk0), 0);
		int n_whole = 0, n_split = 0;
		for(int32_t g = 0; g < br.n_bwd_groups; ++ g) {
			const TSimtBranchGroup &grp = R.simt_bwd_br_groups[size_t(br.n_bwd_first + g)], &grp_factor = R.simt_br_groups[size_t(br.n_first + g)];
			REQUIRE(grp.seg[0].n_tasks > 0);
			for(int k = 0; k < 3; ++ k) {
				REQUIRE(grp.seg[k].n_tasks == grp_factor.seg[k].n_tasks); // the factor form's items, in its order
				if(grp.seg[k].n_tasks > 0) {
					REQUIRE(grp.seg[k].n_tasks <= W && columns_from_segment(R, grp.seg[k], W, 0, cols));
					const int32_t *p_seg = &R.simt_bwd_prog[size_t(grp.seg[k].prog_off)];
					REQUIRE((3 * p_seg[0] + p_seg[1]) * W <= br.n_bwd_tab_region); // the table fits its LDS region
				}
			}
			int n_same_chunk[2] = {-1, -1};
			for(int k = 0; k < 2; ++ k) {
				for(int32_t n_chunk = n_chunk0; n_chunk < n_chunk1 && grp.seg[k].n_tasks > 0; ++ n_chunk) {
					if(R.simt_bwd_chunks[size_t(n_chunk)].tab_off == grp.seg[k].tab_off)
						n_same_chunk[k] = n_chunk;
				}
			}
			const bool b_whole = n_same_chunk[0] >= 0;
			if(b_whole) {
				REQUIRE(grp.seg[2].n_tasks == 0 && (grp.seg[1].n_tasks == 0 || n_same_chunk[1] >= 0));
				c.reached.insert((grp.seg[1].n_tasks == 0)? "single_whole_chunk" : "pair_of_whole_chunks");
			} else {
				REQUIRE(n_same_chunk[1] < 0 && grp.seg[1].n_tasks == grp.seg[0].n_tasks && (grp.seg[2].n_tasks == 0 || grp.seg[2].n_tasks == grp.seg[0].n_tasks));
				++ n_split;
				if(grp.seg[0].n_tasks < W)
					c.reached.insert("split_spare_lanes");
			}
			for(int n_lane = 0; n_lane < grp.seg[0].n_tasks || n_lane < grp.seg[1].n_tasks; ++ n_lane) {
				std::vector<TBwdColumn> seg_cols[3];
				for(int n_half = 0; n_half < (b_whole? 2 : 1); ++ n_half) { // a split task, or a task of either whole chunk
					std::map<int32_t, int> seg_of_col;
					int32_t n_task = -1;
					for(int k = 0; k < 3; ++ k)
						seg_cols[k].clear();
					for(int k = b_whole? n_half : 0; k < (b_whole? n_half + 1 : 3); ++ k) {
						if(n_lane >= grp.seg[k].n_tasks)
							continue;
						REQUIRE(columns_from_segment(R, grp.seg[k], W, n_lane, seg_cols[k]));
						for(size_t i = 0; i < seg_cols[k].size(); ++ i) {
							const int64_t cs = seg_cols[k][i].cs_new;
							REQUIRE(cs >= 0 && size_t(cs) < col_of_cs.size() && col_of_cs[size_t(cs)] >= 0);
							const int32_t j = col_of_cs[size_t(cs)];
							REQUIRE(n_task < 0 || task_of_col[size_t(j)] == n_task); // the same task in this lane of all three
							n_task = task_of_col[size_t(j)];
							REQUIRE(seg_of_col.insert(std::make_pair(j, k)).second); // in exactly one segment
						}
					}
					if(n_task < 0)
						continue; // (the odd whole chunk's missing partner, or the shorter chunk of a pair)
					const int32_t *p_task = &P.task_cols[size_t(P.task_ptr[n_task])];
					const int32_t n_task_cols = int32_t(P.task_ptr[n_task + 1] - P.task_ptr[n_task]);
					REQUIRE(int32_t(seg_of_col.size()) == n_task_cols); // every column of the task
					REQUIRE(n_task_cols * D * W <= br.n_bwd_x_region);
					if(n_lane == 0) {
						REQUIRE(chunk_of_first_task.count(n_task));
						const int32_t n_chunk = chunk_of_first_task[n_task];
						REQUIRE(!chunk_seen[size_t(n_chunk - n_chunk0)] && R.simt_bwd_chunks[size_t(n_chunk)].n_tasks == grp.seg[b_whole? n_half : 0].n_tasks);
						REQUIRE(!b_whole || n_chunk == n_same_chunk[n_half]);
						chunk_seen[size_t(n_chunk - n_chunk0)] = 1;
						n_whole += b_whole;
					}
					std::vector<char> place_seen(size_t(n_task_cols), 0);
					for(int k = 0; k < 3; ++ k) {
						for(size_t i = 0; i < seg_cols[k].size(); ++ i) {
							const TBwdColumn &r_col = seg_cols[k][i];
							const int32_t j = col_of_cs[size_t(r_col.cs_new)];
							REQUIRE(r_col.n_place < n_task_cols && p_task[r_col.n_place] == j && !place_seen[size_t(r_col.n_place)]); // its own place: a permutation
							place_seen[size_t(r_col.n_place)] = 1;
							REQUIRE(i == 0 || seg_cols[k][i - 1].n_place < r_col.n_place); // in the task's order
							REQUIRE(r_col.l_base == P.loff[size_t(P.lptr[j])] && r_col.cs_src == P.cs_src[j] && int64_t(r_col.x_off.size()) == P.lptr[j + 1] - P.lptr[j] - 1);
							int n_outside = 0;
							for(size_t kb = 0; kb < r_col.x_off.size(); ++ kb) {
								const int32_t n_row = P.lrow[size_t(P.lptr[j]) + 1 + kb];
								REQUIRE(r_col.x_off[kb] == P.cs_new[n_row]);
								if(task_of_col[size_t(n_row)] == n_task) {
									REQUIRE(r_col.n_local[kb] > r_col.n_place && r_col.n_local[kb] < n_task_cols && p_task[r_col.n_local[kb]] == n_row); // the task's numbering
									const int n_from = seg_of_col[n_row];
									REQUIRE(b_whole || n_from == k || n_from == 2); // a row inside the task: the same bin, or a join
									REQUIRE(k != 2 || n_from == 2);                 // and a join's: a join
								} else {
									REQUIRE(r_col.n_local[kb] == -1 && task_of_col[size_t(n_row)] >= P.stage_ptr[s + 1]); // (a later stage's: solved by an earlier launch)
									++ n_outside;
								}
							}
							if(n_outside >= 2)
								c.reached.insert("two_rows_outside");
							if(!b_whole && int(r_col.x_off.size()) > int(SIMT_BWD_AHEAD))
								c.reached.insert("segment_column_beyond_the_set");
						}
					}
					if(!b_whole) {
						std::vector<int32_t> parent;
						TSimtSegments t_segs;
						simt_task_parents(P, n_task, parent);
						simt_task_segments(parent, t_segs);
						REQUIRE(t_segs.n_tips >= 2);
						for(int k = 0; k < 3; ++ k) {
							REQUIRE(t_segs.seg[k].size() == seg_cols[k].size());
							for(size_t i = 0; i < seg_cols[k].size(); ++ i)
								REQUIRE(t_segs.seg[k][i] == seg_cols[k][i].n_place);
						}
						c.reached.insert((t_segs.n_tips == 2)? "split_two_tips" : "split_three_tips");
						c.reached.insert((seg_cols[2].size() == 1)? "one_join" : (seg_cols[2].size() == 2)? "two_joins" : (seg_cols[2].empty()? "no_join" : "more_joins"));
					}
					// the numbers: the joins, then bin 0, then bin 1 (the waves run the bins side by side: neither reads the other's x),
					// columns last to first, x of the task's own columns by place
					x_own.assign(size_t(n_task_cols) * size_t(D), -7.0);
					const int order_split[3] = {2, 0, 1};
					for(int n_at = 0; n_at < 3; ++ n_at) {
						const int k = order_split[n_at];
						if(b_whole && k != n_half)
							continue;
						for(size_t i = seg_cols[k].size(); i -- > 0;)
							backward_column(D, seg_cols[k][i], L, w_rec, x_rec, x_own);
					}
				}
			}
		}
		for(size_t i = 0; i < chunk_seen.size(); ++ i)
			REQUIRE(chunk_seen[i]); // every chunk, exactly once
		REQUIRE(n_whole == br.n_whole_chunks && n_split == br.n_split_chunks && br.n_bwd_groups == n_split + (n_whole + 1) / 2);
		if(n_whole % 2)
			c.reached.insert("odd_whole_chunks");
		if(br.n_bwd_spare_chunks > 0)
			c.reached.insert("spare_lanes");
	}
	REQUIRE(memcmp(w_plan.data(), w_rec.data(), w_rec.size() * sizeof(double)) == 0);
	REQUIRE(memcmp(x_plan.data(), x_rec.data(), x_rec.size() * sizeof(double)) == 0);
	bool b_moved = false;
	for(size_t i = 0; i < x_rec.size(); ++ i)
		b_moved = b_moved || x_rec[i] != -7.0;
	REQUIRE(b_moved);
	return true;
}

template <class T>
static bool same_bytes(const T &r_a, const T &r_b, size_t n)
{
	return r_a.size() >= n && r_b.size() >= n && (!n || memcmp(&r_a[0], &r_b[0], n * sizeof(r_a[0])) == 0);
}

static bool build(const char *name, int n, const CEdgeList &edges, int n_leaf_size, int n_width, TCase &c)
{
	const SparseRecordOptions t_opt = {-1, 1, 1, n_width, 1, 8192, true, false}; // (simt = 1: the leaf stage by the lane-per-task kernels at any size)
	c.opt = t_opt;
	PlanOptions plan_opt;
	plan_opt.subtree_size = 8;
	plan_opt.leaf_size = n_leaf_size;
	plan_opt.dense_top_nb = 0;
	plan_opt.task_wide_min = std::max(t_opt.n_wide_min_tasks, 1);
	plan_opt.task_max_cols = int(PANEL_COLS);
	plan_opt.task_max_blocks = panel_slot_cap(6);
	if(!plan_of_graph(name, n, edges, std::vector<int>(1, 6), plan_opt, c.P))
		return false;
	c.L.n_bottom_stages = count_bottom_stages(c.P, c.opt);
	build_simt_tables(c.P, c.opt, c.R, c.L);
	return true;
}

static void set_knobs(const char *p_s_factor, const char *p_s_backward)
{
	if(p_s_factor) setenv("SLAMPP_HIP_DEV_SIMT_FACTOR_BRANCHES", p_s_factor, 1); else unsetenv("SLAMPP_HIP_DEV_SIMT_FACTOR_BRANCHES");
	if(p_s_backward) setenv("SLAMPP_HIP_DEV_SIMT_BWD_BRANCHES", p_s_backward, 1); else unsetenv("SLAMPP_HIP_DEV_SIMT_BWD_BRANCHES");
	dev_knobs_refresh();
}

static bool run(const std::string &s_name, int n, const CEdgeList &edges, int n_leaf_size, int n_width)
{
	const char *name = s_name.c_str();
	TCase c, c_none;
	set_knobs("0", "1"); // every shape with two bins splits, by the backward form's knob alone
	if(!build(name, n, edges, n_leaf_size, n_width, c) || !check(name, c))
		return false;
	set_knobs("0", 0); // no records at all
	if(!build(name, n, edges, n_leaf_size, n_width, c_none))
		return false;
	REQUIRE(c_none.R.simt_br_groups.empty() && c_none.R.simt_bwd_br_groups.empty() && !c.R.simt_bwd_br_groups.empty());
	REQUIRE(c.R.simt_chunks.size() == c_none.R.simt_chunks.size() && same_bytes(c.R.simt_chunks, c_none.R.simt_chunks, c_none.R.simt_chunks.size()));
	REQUIRE(c.R.simt_bwd_chunks.size() == c_none.R.simt_bwd_chunks.size() && same_bytes(c.R.simt_bwd_chunks, c_none.R.simt_bwd_chunks, c_none.R.simt_bwd_chunks.size()));
	REQUIRE(c.R.simt_rest == c_none.R.simt_rest);
	REQUIRE(same_bytes(c.R.simt_prog, c_none.R.simt_prog, c_none.R.simt_prog.size()) && same_bytes(c.R.simt_tab, c_none.R.simt_tab, c_none.R.simt_tab.size()));
	REQUIRE(c.R.simt_bwd_prog.size() > c_none.R.simt_bwd_prog.size() && same_bytes(c.R.simt_bwd_prog, c_none.R.simt_bwd_prog, c_none.R.simt_bwd_prog.size()));
	REQUIRE(c.R.simt_bwd_tab.size() > c_none.R.simt_bwd_tab.size() && same_bytes(c.R.simt_bwd_tab, c_none.R.simt_bwd_tab, c_none.R.simt_bwd_tab.size()));
	REQUIRE(c.L.simt_lds_bytes == c_none.L.simt_lds_bytes && c.L.simt_bwd_lds_bytes == c_none.L.simt_bwd_lds_bytes && c.L.simt_chunk_ptr == c_none.L.simt_chunk_ptr);
	printf("%s: columns %d records %zu reached", name, c.P.n, c.R.simt_bwd_br_groups.size());
	for(std::set<std::string>::const_iterator p = c.reached.begin(); p != c.reached.end(); ++ p)
		printf(" %s", p->c_str());
	printf(" ok\n");
	return true;
}

int main()
{
	setenv("SLAMPP_HIP_DEV", "1", 1); // (the development knobs are read only with it: plan.h)
	std::mt19937 rng(7);
	bool b_ok = true;
	const int leaf_sizes[] = {1, 3}, widths[] = {32, 16};
	const CEdgeList chain300 = chain_with_closures(300, rng), chain612 = chain_with_closures(612, rng);
	CEdgeList hub = chain_with_closures(300, rng); // (tests/variant_util.py: hub_chain)
	for(int i = 10; i < 70; ++ i)
		hub.push_back(std::make_pair(i, 300));
	for(int i = 180; i < 260; ++ i) {
		hub.push_back(std::make_pair(i, i + 2));
		hub.push_back(std::make_pair(i, i + 3));
	}
	CEdgeList islands = chain_with_closures(400, rng); // (tests/test_factor_simt_ahead_gpu.py: islands) 40 single poses, 40 pairs, 40 paths of three
	int n_islands = 400;
	for(int n_size = 1; n_size <= 3; ++ n_size) {
		for(int i = 0; i < 40; ++ i, n_islands += n_size) {
			for(int k = 1; k < n_size; ++ k)
				islands.push_back(std::make_pair(n_islands + k - 1, n_islands + k));
		}
	}
	for(int l = 0; l < 2; ++ l) {
		for(int w = 0; w < 2; ++ w) {
			const std::string s_tail = "-leaf" + std::to_string(leaf_sizes[l]) + "-w" + std::to_string(widths[w]);
			b_ok = run("chain300" + s_tail, 300, chain300, leaf_sizes[l], widths[w]) && b_ok;
			b_ok = run("chain612" + s_tail, 612, chain612, leaf_sizes[l], widths[w]) && b_ok;
			b_ok = run("hub" + s_tail, 301, hub, leaf_sizes[l], widths[w]) && b_ok;
			b_ok = run("islands" + s_tail, n_islands, islands, leaf_sizes[l], widths[w]) && b_ok;
		}
	}
	return b_ok? 0 : 1;
}
