// Test infrastructure (see tests/test_simt_branches_host.py): the workgroup records of the two-wave leaf factor form
// (csrc/sparse_kernels.h: TSimtBranchGroup; csrc/sparse_records.cpp: simt_task_segments(), Build_Simt_Branches()) on the CPU.
// The driver builds plan and lane-per-task tables of a few graphs with every two-bin shape split, and checks of every split
// task that its columns lie in exactly one segment each, that whatever a column reads of its own task was produced earlier in
// the same segment or -- for the join segment -- in either bin, that no bin reads from the other bin or from the joins, and
// that the three segments hold the same task in the same lane; of every stage that its records cover every chunk exactly
// once.  It then runs the factorization with the fused forward substitution twice in plain C++ with one column routine: task
// by task from the Plan, and record by record from the segments' programs and tables alone (segment 0, segment 1, segment 2),
// and requires L, inv(L_jj) and w equal element for element.
#include "sparse_records.h"
#include "driver_graphs.h"
#include <cmath>
#include <cstring>
#include <map>
#include <string>

using namespace slampp;

#define REQUIRE(cond) do { if(!(cond)) { printf("%s: failed: %s (line %d)\n", name, #cond, __LINE__); return false; } } while(0)

struct TNumbers {
	std::vector<double> A, b, L, Linv, w;
};

// what one column reads and writes, as offsets
struct TColumnJob {
	int64_t l_base, linv_off, cs_new, cs_src;
	std::vector<int64_t> enc;                                // per block of the column: (offset << 1) | transposed, or -1
	std::vector<std::pair<int64_t, int64_t> > rows;          // row entries: offset of L(j,c), scalar offset of y_c
	std::vector<std::vector<std::pair<int64_t, int64_t> > > pairs; // per block below the diagonal: offsets of L(i,c), L(j,c)
};

// one column in the kernels' order of operations (csrc/simt_factor_ahead.hip: factor_ahead_columns())
static void factor_column(int D, const TColumnJob &c, TNumbers &N)
{
	const int DD = D * D;
	double a[8][8] = {{0}}, y[8], x[8][8], rd[8];
	for(int r = 0; r < D; ++ r) {
		for(int q = 0; q <= r; ++ q)
			a[r][q] = (c.enc[0] >= 0)? N.A[size_t((c.enc[0] >> 1) + q + r * D)] : 0.0; // element (r, q), r >= q, is stored element (q, r)
		y[r] = N.b[size_t(c.cs_src + r)];
	}
	for(size_t e = 0; e < c.rows.size(); ++ e) {
		const double *blk = &N.L[size_t(c.rows[e].first)], *yc = &N.w[size_t(c.rows[e].second)];
		for(int t = 0; t < D; ++ t) {
			for(int r = 0; r < D; ++ r) {
				for(int q = 0; q <= r; ++ q)
					a[r][q] -= blk[r + t * D] * blk[q + t * D];
				y[r] -= blk[r + t * D] * yc[t];
			}
		}
	}
	for(int k = 0; k < D; ++ k) {
		double piv = a[k][k];
		if(!(piv > 0))
			piv = 1.0;
		const double s = 1.0 / sqrt(piv);
		rd[k] = s;
		a[k][k] = piv * s;
		for(int r = k + 1; r < D; ++ r)
			a[r][k] *= s;
		for(int q = k + 1; q < D; ++ q) {
			for(int r = q; r < D; ++ r)
				a[r][q] -= a[r][k] * a[q][k];
		}
	}
	for(int cc = 0; cc < D; ++ cc) {
		for(int r = 0; r < D; ++ r) {
			if(r < cc)
				x[r][cc] = 0.0;
			else if(r == cc)
				x[r][cc] = rd[r];
			else {
				double sum = 0;
				for(int t = cc; t < r; ++ t)
					sum += a[r][t] * x[t][cc];
				x[r][cc] = -sum * rd[r];
			}
		}
	}
	for(int r = 0; r < D; ++ r) {
		double sum = 0;
		for(int t = 0; t <= r; ++ t)
			sum += x[r][t] * y[t];
		N.w[size_t(c.cs_new + r)] = sum;
	}
	for(int r = 0; r < D; ++ r) {
		for(int q = 0; q < D; ++ q) {
			N.L[size_t(c.l_base + r + q * D)] = (q <= r)? a[r][q] : 0.0;
			N.Linv[size_t(c.linv_off + r + q * D)] = x[r][q];
		}
	}
	for(size_t kb = 1; kb < c.enc.size(); ++ kb) {
		double acc[8][8];
		const int64_t enc = c.enc[kb];
		for(int i = 0; i < D; ++ i) {
			for(int q = 0; q < D; ++ q)
				acc[i][q] = (enc < 0)? 0.0 : N.A[size_t((enc >> 1) + ((enc & 1)? q + i * D : i + q * D))];
		}
		for(size_t e = 0; e < c.pairs[kb - 1].size(); ++ e) {
			const double *ca = &N.L[size_t(c.pairs[kb - 1][e].first)], *cb = &N.L[size_t(c.pairs[kb - 1][e].second)];
			for(int t = 0; t < D; ++ t) {
				for(int i = 0; i < D; ++ i) {
					for(int q = 0; q < D; ++ q)
						acc[i][q] -= ca[i + t * D] * cb[q + t * D];
				}
			}
		}
		for(int q = 0; q < D; ++ q) {
			for(int i = 0; i < D; ++ i) {
				double sum = 0;
				for(int t = 0; t <= q; ++ t)
					sum += acc[i][t] * x[q][t];
				N.L[size_t(c.l_base + int64_t(kb) * DD + i + q * D)] = sum;
			}
		}
	}
}

static void column_job_from_plan(const Plan &P, int32_t j, TColumnJob &c)
{
	c.l_base = P.loff[P.lptr[j]]; c.linv_off = P.linv_off[j]; c.cs_new = P.cs_new[j]; c.cs_src = P.cs_src[j];
	c.enc.clear(); c.rows.clear(); c.pairs.clear();
	for(int64_t k = P.lptr[j]; k < P.lptr[j + 1]; ++ k)
		c.enc.push_back((P.asrc[k] < 0)? -1 : P.asrc[k] * 2 + P.atrans[k]);
	for(int64_t e = P.rptr[j]; e < P.rptr[j + 1]; ++ e)
		c.rows.push_back(std::make_pair(P.loff[P.rblk[e]], P.cs_new[P.blk_col[P.rblk[e]]]));
	for(int64_t k = P.lptr[j] + 1; k < P.lptr[j + 1]; ++ k) {
		c.pairs.push_back(std::vector<std::pair<int64_t, int64_t> >());
		for(int64_t e = P.pptr[k]; e < P.pptr[k + 1]; ++ e)
			c.pairs.back().push_back(std::make_pair(P.loff[P.pa[e]], P.loff[P.pb[e]]));
	}
}

// the columns of one lane of a chunk, from its program and table alone; false: the program or the table is malformed
static bool column_jobs_from_chunk(const SparseRecords &R, const TSimtChunk &ch, int W, int n_lane, std::vector<TColumnJob> &jobs)
{
	jobs.clear();
	if(ch.prog_off < 0 || size_t(ch.prog_off) + 4 > R.simt_prog.size())
		return false;
	const int32_t *P = &R.simt_prog[size_t(ch.prog_off)];
	const int n_cols = P[0], n_blocks = P[1], n_ops = P[2], n_ys = P[3], n_fields = 4 * n_cols + n_blocks + n_ops + n_ys;
	if(ch.tab_off < 0 || size_t(ch.tab_off) + size_t(n_fields) * size_t(W) > R.simt_tab.size())
		return false;
	const int64_t *T = &R.simt_tab[size_t(ch.tab_off)] + n_lane;
	const int f_blk = 4 * n_cols, f_op = f_blk + n_blocks, f_y = f_op + n_ops;
	size_t pc = 4;
	int blk0 = 0;
	const size_t n_prog_end = R.simt_prog.size() - size_t(ch.prog_off);
	for(int ci = 0; ci < n_cols; ++ ci) {
		if(pc + 3 > n_prog_end)
			return false;
		const int nb = P[pc], nr = P[pc + 1], n_touch = P[pc + 2];
		pc += 3 + size_t(n_touch);
		if(nb < 1 || nr < 0 || n_touch < 0 || blk0 + nb > n_blocks || pc + 2 * size_t(nr) > n_prog_end)
			return false;
		TColumnJob c;
		c.l_base = T[W * (4 * ci)]; c.linv_off = T[W * (4 * ci + 1)]; c.cs_new = T[W * (4 * ci + 2)]; c.cs_src = T[W * (4 * ci + 3)];
		for(int k = 0; k < nb; ++ k)
			c.enc.push_back(T[W * (f_blk + blk0 + k)]);
		for(int e = 0; e < nr; ++ e, pc += 2) {
			if(P[pc] < 0 || P[pc] >= n_ops || P[pc + 1] < 0 || P[pc + 1] >= n_ys)
				return false;
			c.rows.push_back(std::make_pair(T[W * (f_op + P[pc])], T[W * (f_y + P[pc + 1])]));
		}
		for(int kb = 1; kb < nb; ++ kb) {
			if(pc + 1 > n_prog_end)
				return false;
			const int np = P[pc ++];
			if(np < 0 || pc + 2 * size_t(np) > n_prog_end)
				return false;
			c.pairs.push_back(std::vector<std::pair<int64_t, int64_t> >());
			for(int e = 0; e < np; ++ e, pc += 2) {
				if(P[pc] < 0 || P[pc] >= n_ops || P[pc + 1] < 0 || P[pc + 1] >= n_ops)
					return false;
				c.pairs.back().push_back(std::make_pair(T[W * (f_op + P[pc])], T[W * (f_op + P[pc + 1])]));
			}
		}
		blk0 += nb;
		jobs.push_back(c);
	}
	// the trailing list, per block below a diagonal which of the chunk's columns its row is: relative to these columns
	for(int ci = 0; ci < n_cols; ++ ci) {
		for(size_t kb = 1; kb < jobs[size_t(ci)].enc.size(); ++ kb, ++ pc) {
			if(pc >= n_prog_end || P[pc] < -1 || P[pc] >= n_cols || (P[pc] >= 0 && P[pc] <= ci))
				return false;
		}
	}
	return blk0 == n_blocks;
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
	const int64_t n_lblocks = int64_t(P.lrow.size());
	REQUIRE(P.uniform_dim && D == 6 && P.dense_dim == 0);
	REQUIRE(!c.L.simt_chunk_ptr.empty() && c.L.simt_br.size() + 1 == c.L.simt_chunk_ptr.size());
	std::vector<int32_t> col_of_cs(size_t(P.cs_new[P.n]) + 1, -1), task_of_col(size_t(P.n), -1);
	std::map<int64_t, int32_t> col_of_loff; // offset of a factor block -> the column it lies in
	for(int32_t j = 0; j < P.n; ++ j) {
		col_of_cs[size_t(P.cs_new[j])] = j;
		for(int64_t k = P.lptr[j]; k < P.lptr[j + 1]; ++ k)
			col_of_loff[P.loff[k]] = j;
	}
	const int n_stages = int(P.stage_ptr.size()) - 1;
	for(int t = 0; t < P.stage_ptr[n_stages]; ++ t) {
		for(int64_t i = P.task_ptr[t]; i < P.task_ptr[t + 1]; ++ i)
			task_of_col[size_t(P.task_cols[size_t(i)])] = t;
	}
	// fixed pseudo-random numbers: small blocks, heavy diagonals
	TNumbers N0;
	int64_t n_a_size = 0;
	for(int64_t k = 0; k < n_lblocks; ++ k)
		n_a_size = std::max(n_a_size, (P.asrc[size_t(k)] < 0)? 0 : P.asrc[size_t(k)] + D * D);
	N0.A.resize(size_t(n_a_size));
	N0.b.resize(size_t(P.cs_new[P.n]));
	uint64_t n_state = 0x9e3779b97f4a7c15ull;
	auto Next = [&]() { n_state = n_state * 6364136223846793005ull + 1442695040888963407ull; return double(int64_t(n_state >> 11) % 2000001 - 1000000) * 1e-6; };
	for(size_t i = 0; i < N0.A.size(); ++ i) N0.A[i] = 0.05 * Next();
	for(size_t i = 0; i < N0.b.size(); ++ i) N0.b[i] = Next();
	for(int32_t j = 0; j < P.n; ++ j) {
		REQUIRE(P.asrc[size_t(P.lptr[j])] >= 0);
		for(int q = 0; q < D; ++ q)
			N0.A[size_t(P.asrc[size_t(P.lptr[j])] + q + q * D)] += 12.0;
	}
	N0.L.assign(size_t(P.loff[size_t(n_lblocks)]), -7.0);
	N0.Linv.assign(size_t(P.linv_off[size_t(P.n)]), -7.0);
	N0.w.assign(size_t(P.cs_new[P.n]), -7.0);
	TNumbers N_plan(N0), N_rec(N0);
	std::vector<TColumnJob> jobs;
	for(size_t s = 0; s + 1 < c.L.simt_chunk_ptr.size(); ++ s) {
		const TSimtBranchStage &br = c.L.simt_br[s];
		REQUIRE(br.n_groups > 0 && size_t(br.n_first + br.n_groups) <= R.simt_br_groups.size() && br.n_lds_bytes > 0 && br.n_lds_bytes <= 64 * 1024);
		const int32_t n_chunk0 = c.L.simt_chunk_ptr[s], n_chunk1 = c.L.simt_chunk_ptr[s + 1];
		// run A: the stage's lane-per-task tasks one by one from the Plan
		std::map<int32_t, int32_t> chunk_of_first_task;
		for(int32_t n_chunk = n_chunk0; n_chunk < n_chunk1; ++ n_chunk) {
			const TSimtChunk &ch = R.simt_chunks[size_t(n_chunk)];
			REQUIRE(ch.n_tasks >= 1 && ch.n_tasks <= W);
			if(ch.n_tasks < W)
				c.reached.insert("spare_lanes");
			for(int n_lane = 0; n_lane < ch.n_tasks; ++ n_lane) {
				REQUIRE(column_jobs_from_chunk(R, ch, W, n_lane, jobs) && !jobs.empty());
				const int32_t t = task_of_col[size_t(col_of_cs[size_t(jobs[0].cs_new)])];
				if(n_lane == 0)
					chunk_of_first_task[t] = n_chunk;
				TColumnJob t_job;
				for(int64_t i = P.task_ptr[t]; i < P.task_ptr[t + 1]; ++ i) {
					column_job_from_plan(P, P.task_cols[size_t(i)], t_job);
					factor_column(D, t_job, N_plan);
				}
			}
		}
		// run B: record by record, segment by segment
		std::vector<char> chunk_seen(size_t(n_chunk1 - n_chunk0), 0);
		int n_whole = 0, n_split = 0, n_split_tasks = 0, n_longest = 0;
		for(int32_t g = br.n_first; g < br.n_first + br.n_groups; ++ g) {
			const TSimtBranchGroup &grp = R.simt_br_groups[size_t(g)];
			REQUIRE(grp.seg[0].n_tasks > 0);
			int n_same_chunk[2] = {-1, -1};
			for(int k = 0; k < 2; ++ k) {
				for(int32_t n_chunk = n_chunk0; n_chunk < n_chunk1 && grp.seg[k].n_tasks > 0; ++ n_chunk) {
					const TSimtChunk &ch = R.simt_chunks[size_t(n_chunk)];
					if(ch.prog_off == grp.seg[k].prog_off && ch.tab_off == grp.seg[k].tab_off && ch.n_tasks == grp.seg[k].n_tasks)
						n_same_chunk[k] = n_chunk;
				}
			}
			const bool b_whole = n_same_chunk[0] >= 0;
			int n_chain = 0;
			if(b_whole) { // chunks of whole tasks, one or two
				REQUIRE(grp.seg[2].n_tasks == 0 && (grp.seg[1].n_tasks == 0 || n_same_chunk[1] >= 0));
				if(grp.seg[1].n_tasks == 0)
					c.reached.insert("single_whole_chunk");
				else
					c.reached.insert("pair_of_whole_chunks");
				for(int k = 0; k < 2; ++ k) {
					if(n_same_chunk[k] < 0)
						continue;
					REQUIRE(!chunk_seen[size_t(n_same_chunk[k] - n_chunk0)]);
					chunk_seen[size_t(n_same_chunk[k] - n_chunk0)] = 1;
					++ n_whole;
					n_chain = std::max(n_chain, int(R.simt_prog[size_t(grp.seg[k].prog_off)]));
					for(int n_lane = 0; n_lane < grp.seg[k].n_tasks; ++ n_lane) {
						REQUIRE(column_jobs_from_chunk(R, grp.seg[k], W, n_lane, jobs));
						for(size_t i = 0; i < jobs.size(); ++ i)
							factor_column(D, jobs[i], N_rec);
					}
					c.reached.insert("whole_task");
				}
			} else {
				REQUIRE(grp.seg[1].n_tasks == grp.seg[0].n_tasks && (grp.seg[2].n_tasks == 0 || grp.seg[2].n_tasks == grp.seg[0].n_tasks));
				++ n_split;
				n_split_tasks += grp.seg[0].n_tasks;
				for(int k = 0; k < 3; ++ k)
					REQUIRE(grp.seg[k].n_tasks == 0 || int(4 * R.simt_prog[size_t(grp.seg[k].prog_off)] + R.simt_prog[size_t(grp.seg[k].prog_off) + 1] +
						R.simt_prog[size_t(grp.seg[k].prog_off) + 2] + R.simt_prog[size_t(grp.seg[k].prog_off) + 3]) * W * 8 * 2 <= br.n_lds_bytes);
				const int n_bin0 = R.simt_prog[size_t(grp.seg[0].prog_off)], n_bin1 = R.simt_prog[size_t(grp.seg[1].prog_off)],
					n_joins = (grp.seg[2].n_tasks > 0)? R.simt_prog[size_t(grp.seg[2].prog_off)] : 0;
				n_chain = std::max(n_bin0, n_bin1) + n_joins;
				REQUIRE(n_bin0 >= n_bin1 && n_bin1 >= 1);
				if(n_bin1 == 1)
					c.reached.insert("one_column_bin");
				if(n_joins == 2)
					c.reached.insert("two_column_joins");
				for(int n_lane = 0; n_lane < grp.seg[0].n_tasks; ++ n_lane) {
					std::map<int32_t, int> seg_of_col; // the task's columns -> their segment
					int32_t n_task = -1;
					std::vector<TColumnJob> seg_jobs[3];
					for(int k = 0; k < 3; ++ k) {
						if(grp.seg[k].n_tasks == 0)
							continue;
						REQUIRE(column_jobs_from_chunk(R, grp.seg[k], W, n_lane, seg_jobs[k]));
						for(size_t i = 0; i < seg_jobs[k].size(); ++ i) {
							const int64_t cs = seg_jobs[k][i].cs_new;
							REQUIRE(cs >= 0 && size_t(cs) < col_of_cs.size() && col_of_cs[size_t(cs)] >= 0);
							const int32_t j = col_of_cs[size_t(cs)];
							REQUIRE(n_task < 0 || task_of_col[size_t(j)] == n_task); // the same task in this lane of all three
							n_task = task_of_col[size_t(j)];
							REQUIRE(seg_of_col.insert(std::make_pair(j, k)).second); // in exactly one segment
							TColumnJob t_ref;
							column_job_from_plan(P, j, t_ref);
							REQUIRE(t_ref.l_base == seg_jobs[k][i].l_base && t_ref.linv_off == seg_jobs[k][i].linv_off && t_ref.cs_src == seg_jobs[k][i].cs_src &&
								t_ref.enc == seg_jobs[k][i].enc && t_ref.rows == seg_jobs[k][i].rows && t_ref.pairs == seg_jobs[k][i].pairs);
						}
					}
					REQUIRE(n_task >= 0 && int64_t(seg_of_col.size()) == P.task_ptr[n_task + 1] - P.task_ptr[n_task]);
					if(n_lane == 0) {
						REQUIRE(chunk_of_first_task.count(n_task));
						const int32_t n_chunk = chunk_of_first_task[n_task];
						REQUIRE(!chunk_seen[size_t(n_chunk - n_chunk0)] && R.simt_chunks[size_t(n_chunk)].n_tasks == grp.seg[0].n_tasks);
						chunk_seen[size_t(n_chunk - n_chunk0)] = 1;
					}
					std::vector<int32_t> parent;
					TSimtSegments t_segs;
					simt_task_parents(P, n_task, parent);
					REQUIRE(simt_task_segments(parent, t_segs) == n_chain && t_segs.n_tips >= 2);
					c.reached.insert((t_segs.n_tips == 2)? "split_two_tips" : (t_segs.n_tips == 3)? "split_three_tips" : "split_more_tips");
					// what every column reads of its own task: produced earlier in the same segment, or, for the joins, in a bin
					for(int k = 0; k < 3; ++ k) {
						std::set<int32_t> done; // the columns of this segment so far
						for(size_t i = 0; i < seg_jobs[k].size(); ++ i) {
							const TColumnJob &r_job = seg_jobs[k][i];
							std::vector<int32_t> reads;
							for(size_t e = 0; e < r_job.rows.size(); ++ e) {
								REQUIRE(col_of_loff.count(r_job.rows[e].first) && col_of_cs[size_t(r_job.rows[e].second)] >= 0);
								reads.push_back(col_of_loff[r_job.rows[e].first]);
								reads.push_back(col_of_cs[size_t(r_job.rows[e].second)]);
							}
							for(size_t kb = 0; kb < r_job.pairs.size(); ++ kb) {
								for(size_t e = 0; e < r_job.pairs[kb].size(); ++ e) {
									REQUIRE(col_of_loff.count(r_job.pairs[kb][e].first) && col_of_loff.count(r_job.pairs[kb][e].second));
									reads.push_back(col_of_loff[r_job.pairs[kb][e].first]);
									reads.push_back(col_of_loff[r_job.pairs[kb][e].second]);
								}
							}
							for(size_t e = 0; e < reads.size(); ++ e) {
								if(task_of_col[size_t(reads[e])] != n_task) {
									REQUIRE(task_of_col[size_t(reads[e])] < P.stage_ptr[s]); // (an earlier stage's)
									continue;
								}
								const int n_from = seg_of_col[reads[e]];
								REQUIRE((n_from == k && done.count(reads[e])) || (k == 2 && n_from < 2));
							}
							done.insert(col_of_cs[size_t(r_job.cs_new)]);
						}
					}
				}
				// the numbers: all lanes' segment 0, then segment 1, then segment 2 (the waves run the first two side by side: neither reads the other's)
				for(int k = 0; k < 3; ++ k) {
					for(int n_lane = 0; n_lane < grp.seg[k].n_tasks; ++ n_lane) {
						REQUIRE(column_jobs_from_chunk(R, grp.seg[k], W, n_lane, jobs));
						for(size_t i = 0; i < jobs.size(); ++ i)
							factor_column(D, jobs[i], N_rec);
					}
				}
			}
			REQUIRE(g == br.n_first || n_chain <= n_longest); // longest first
			if(g == br.n_first)
				n_longest = n_chain;
		}
		for(size_t i = 0; i < chunk_seen.size(); ++ i)
			REQUIRE(chunk_seen[i]); // every chunk, exactly once
		REQUIRE(n_whole == br.n_whole_chunks && n_split == br.n_split_chunks && n_split_tasks == br.n_split_tasks && n_longest == br.n_longest_chain);
		REQUIRE(br.n_groups == n_split + (n_whole + 1) / 2);
		if(n_whole % 2)
			c.reached.insert("odd_whole_chunks");
	}
	REQUIRE(memcmp(N_plan.L.data(), N_rec.L.data(), N_rec.L.size() * sizeof(double)) == 0);
	REQUIRE(memcmp(N_plan.Linv.data(), N_rec.Linv.data(), N_rec.Linv.size() * sizeof(double)) == 0);
	REQUIRE(memcmp(N_plan.w.data(), N_rec.w.data(), N_rec.w.size() * sizeof(double)) == 0);
	bool b_moved = false;
	for(size_t i = 0; i < N_rec.w.size(); ++ i)
		b_moved = b_moved || N_rec.w[i] != -7.0;
	REQUIRE(b_moved);
	return true;
}

static bool run(const std::string &s_name, int n, const CEdgeList &edges, int n_leaf_size, int n_width)
{
	const char *name = s_name.c_str();
	TCase c;
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
	if(!check(name, c))
		return false;
	printf("%s: columns %d records %zu reached", name, c.P.n, c.R.simt_br_groups.size());
	for(std::set<std::string>::const_iterator p = c.reached.begin(); p != c.reached.end(); ++ p)
		printf(" %s", p->c_str());
	printf(" ok\n");
	return true;
}

int main()
{
	setenv("SLAMPP_HIP_DEV", "1", 1); // (the development knobs are read only with it: plan.h)
	setenv("SLAMPP_HIP_DEV_SIMT_FACTOR_BRANCHES", "1", 1); // every shape with two bins splits
	dev_knobs_refresh();
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
