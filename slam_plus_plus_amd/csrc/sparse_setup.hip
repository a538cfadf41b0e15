// sparse_setup.hip -- analysis of the sparse block path: plan, threads, uploads and allocations (cold path); the records the
// kernels read are laid out by the host-only builders of sparse_records.cpp
// (one of the translation units solver.hip was split into in round 5: solver.hip the handle and its device memory,
// staging.hip pinned staging and uploads, sparse_setup.hip the analysis of the sparse block path, sparse_enqueue.hip its launches,
// capi.hip the C ABI of include/slampp_hip.h; the records the analysis lays out are host-only code: sparse_records.cpp, host_pool.cpp)
#include <execinfo.h>
#include <signal.h>
#include <unistd.h>
#include <pthread.h>
#include "solver.h"
#include "sparse_inverse.h"
#include "sparse_records.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <unordered_map>
#include <thread>
#include <mutex>
#include <condition_variable>
#include <functional>
#include <sys/mman.h>

using namespace slampp;

void slampp_hip_solver::Refine_Structure()
{
	const int64_t n = int64_t(cumsum.size()) - 1;
	b_refined = false;
	for(int64_t c = 0; c < n && !b_refined; ++ c)
		b_refined = cumsum[c + 1] - cumsum[c] > 8;
	if(!b_refined) {
		refined_cumsum.clear(); refined_bcol_ptr.clear(); refined_brow.clear();
		d_refine_map.Free(); d_refined.Free();
		n_refined_values = 0;
		return;
	}
	std::vector<int64_t> first_piece(size_t(n) + 1, 0); // pieces of block column c: [first_piece[c], first_piece[c + 1])
	refined_cumsum.assign(1, 0);
	for(int64_t c = 0; c < n; ++ c) {
		const int64_t w = cumsum[c + 1] - cumsum[c], n_pieces = (w + 7) / 8;
		for(int64_t i = 0; i < n_pieces; ++ i)
			refined_cumsum.push_back(cumsum[c] + w * (i + 1) / n_pieces);
		first_piece[c + 1] = first_piece[c] + n_pieces;
	}
	const int64_t n_refined = first_piece[n];
	refined_bcol_ptr.assign(size_t(n_refined) + 1, 0);
	refined_brow.clear();
	std::vector<int64_t> map;
	int64_t n_src_off = 0; // offset of the caller's block (r, c) in the packed values
	std::vector<int64_t> col_src_off; // per block of column c: its offset
	for(int64_t c = 0; c < n; ++ c) {
		const int64_t w = cumsum[c + 1] - cumsum[c];
		col_src_off.clear();
		for(int64_t k = bcol_ptr[c]; k < bcol_ptr[c + 1]; ++ k) {
			col_src_off.push_back(n_src_off);
			n_src_off += (cumsum[brow[k] + 1] - cumsum[brow[k]]) * w;
		}
		for(int64_t pj = first_piece[c]; pj < first_piece[c + 1]; ++ pj) { // refined column pj: rows ascend with the caller's blocks
			const int64_t n_col0 = refined_cumsum[pj] - cumsum[c], n_pw = refined_cumsum[pj + 1] - refined_cumsum[pj];
			for(int64_t k = bcol_ptr[c]; k < bcol_ptr[c + 1]; ++ k) {
				const int64_t r = brow[k], h = cumsum[r + 1] - cumsum[r];
				for(int64_t pi = first_piece[r]; pi < first_piece[r + 1]; ++ pi) {
					if(pi > pj)
						break; // below the diagonal of a diagonal block
					const int64_t n_row0 = refined_cumsum[pi] - cumsum[r], n_ph = refined_cumsum[pi + 1] - refined_cumsum[pi];
					refined_brow.push_back(int32_t(pi));
					for(int64_t b = 0; b < n_pw; ++ b) {
						for(int64_t a = 0; a < n_ph; ++ a)
							map.push_back(col_src_off[size_t(k - bcol_ptr[c])] + (n_row0 + a) + (n_col0 + b) * h);
					}
				}
			}
			refined_bcol_ptr[pj + 1] = int64_t(refined_brow.size());
		}
	}
	n_refined_values = int64_t(map.size());
	Join_Bringup(); // (solver.h: a fresh handle's streams)
	d_refine_map.Upload(map, stream);
	d_refined.Alloc(map.size());
	SLAMPP_HIP_CHECK(hipStreamSynchronize(stream)); // map lives on this stack frame
}

namespace {

// the phases of the analysis on stderr (SLAMPP_HIP_PLAN_TIMING)
struct TSetupPhases {
	bool b_timing;
	double t_phase;
	void operator ()(const char *p_s_name)
	{
		if(b_timing) {
			const double t_now = wall_ms();
			fprintf(stderr, "[setup] %-12s %8.2f ms\n", p_s_name, t_now - t_phase);
			t_phase = t_now;
		}
	}
};

// the plan of the (refined) structure; throws
void Build_Sparse_Plan(slampp_hip_solver &s)
{
	s.Refine_Structure();
	{ // a tall task must fit the panel kernel: its columns and the blocks of its LDS image
		const std::vector<int64_t> &r_cs = s.b_refined? s.refined_cumsum : s.cumsum;
		const int n_dim0 = int(r_cs[1] - r_cs[0]);
		s.opt.task_wide_min = std::max(dev_knob("SLAMPP_HIP_DEV_WIDE_MIN", s.n_wide_min_tasks), 1); // (development aid: overrides the option "wide_min_tasks")
		s.opt.task_max_cols = int(PANEL_COLS);
		s.opt.task_max_blocks = panel_slot_cap(n_dim0);
	}
	std::string s_err = s.b_refined? build_plan(int64_t(s.refined_cumsum.size()) - 1, s.refined_cumsum.data(), s.refined_bcol_ptr.data(),
		s.refined_brow.data(), s.opt, s.plan) : build_plan(int64_t(s.cumsum.size()) - 1, s.cumsum.data(), s.bcol_ptr.data(), s.brow.data(), s.opt, s.plan);
	if(!s_err.empty())
		throw std::invalid_argument(s_err);
	if(s.plan.max_dim > 8)
		throw std::logic_error("a block column wider than 8 survived the refinement");
}

// what the record builders read of the handle (sparse_records.h)
SparseRecordOptions t_Record_Options(const slampp_hip_solver &s, bool b_timing)
{
	SparseRecordOptions t_opt;
	t_opt.n_panel = s.n_panel;
	t_opt.n_panel_handup = s.n_panel_handup;
	t_opt.n_simt = s.n_simt;
	t_opt.n_simt_width = s.n_simt_width;
	t_opt.n_simt_stages = s.n_simt_stages;
	t_opt.n_wide_min_tasks = s.n_wide_min_tasks;
	t_opt.b_small = s.plan.n < 8192; // (small systems -- FastL's parts of R, reduced camera systems -- do their host work on the calling thread: a thread is ~0.1 ms to start, and threads that spin under a CPU quota cost a scheduler period now and then)
	t_opt.b_timing = b_timing;
	return t_opt;
}

// the column records and the column packages: on a thread of their own beside the host work that follows
void Upload_Records(slampp_hip_solver &s, const SparseRecords &r_rec)
{
	s.Join_Bringup(); // (a handle fresh from slampp_hip_create: its streams came up beside the plan and the records -- solver.h)
	SLAMPP_HIP_CHECK(hipSetDevice(s.n_device));
	s.d_cols.Upload(r_rec.cols, s.stream);
	s.d_blks.Upload(r_rec.blks, s.stream);
	s.d_pairs.Upload(r_rec.pairs, s.stream);
	s.d_rents.Upload(r_rec.rents, s.stream);
	s.d_task_ptr.Upload(s.plan.task_ptr, s.stream);
	if(!r_rec.pkg.empty()) {
		s.d_pkg.Upload(r_rec.pkg, s.stream);
		s.d_task_pkg.Upload(r_rec.task_pkg, s.stream);
	} else {
		s.d_pkg.Free();
		s.d_task_pkg.Free();
	}
}

// the dense top's records, its workspaces and its tile schedule
void Setup_Dense_Top(slampp_hip_solver &s, const SparseRecords &r_rec, TSetupPhases &Phase)
{
	const Plan &P = s.plan;
	const int n_dense_pad = s.n_dense_pad;
	Phase("dense records");
	s.d_dense_blks.Upload(r_rec.dense_blks, s.stream);
	s.d_dense_blk_loff.Upload(r_rec.dense_blk_loff, s.stream);
	Phase("dense upload 1");
	s.n_dense_gaps = int(r_rec.gaps.size());
	s.d_dense_gaps.Upload(r_rec.gaps, s.stream);
	s.d_dense_unit.Upload(r_rec.unit, s.stream);
	s.d_dense_dst.Upload(r_rec.dst, s.stream);
	Phase("dense upload 2");
	SLAMPP_HIP_CHECK(hipStreamSynchronize(s.stream));
	Phase("dense lists");
	s.d_dense.Alloc(size_t(n_dense_pad) * n_dense_pad);
	s.b_dense_clean = false;
	s.d_dense_invdiag.Alloc(size_t(n_dense_pad / dense_NB) * dense_NB * dense_NB);
	s.d_dense_z.Alloc(n_dense_pad);
	s.d_dense_x.Alloc(n_dense_pad);
	Phase("dense allocs");
	// which 64 x 64 tiles of the dense top are structurally nonzero, and how long the dependent chain is if only
	// those are touched and independent tile columns are factored side by side
	s.b_dense_tiles = false;
	if(s.n_dense_top_tiles == 0) {
		if(Phase.b_timing)
			fprintf(stderr, "[setup] dense top: %d tiles per side, option dense_top_tiles = 0 -> dense schedule\n", n_dense_pad / dense_NB);
		return;
	}
	std::vector<char> nonzero;
	const int T = dense_top_tile_pattern(P, nonzero);
	if(T != n_dense_pad / dense_NB)
		throw std::logic_error("dense top: tile count mismatch");
	if(s.dense_tiles.Build(T, nonzero, s.stream)) // two launches (26 us) per tile against three (34 us) per level, and fewer tiles touched
		s.b_dense_tiles = s.n_dense_top_tiles > 0 || 100 * s.dense_tiles.n_levels <= 85 * T;
	if(Phase.b_timing) {
		size_t n_nz = 0;
		for(size_t k = 0; k < nonzero.size(); ++ k)
			n_nz += nonzero[k];
		fprintf(stderr, "[setup] dense top: %d tiles per side, %zu of %d lower tiles nonzero before fill, %d levels, "
			"%d trsm tiles, %d update targets -> %s schedule\n", T, n_nz, T * (T + 1) / 2, s.dense_tiles.n_levels,
			s.dense_tiles.level_trsm_ptr.empty()? 0 : s.dense_tiles.level_trsm_ptr.back(),
			s.dense_tiles.level_tgt_ptr.empty()? 0 : s.dense_tiles.level_tgt_ptr.back(), s.b_dense_tiles? "tile" : "dense");
	}
}

} // anonymous namespace

void slampp_hip_solver::Analyze_Sparse()
{
	Join_Discard(); // (the previous analysis' arrays)
	if(p_sinv) { // lists of the previous plan
		sparse_inverse_destroy(p_sinv);
		p_sinv = 0;
	}
	b_sinv_tried = false;
	TSetupPhases Phase = {getenv("SLAMPP_HIP_PLAN_TIMING") != 0, wall_ms()};
	const bool b_timing = Phase.b_timing;

	// 1. plan and options
	Build_Sparse_Plan(*this);
	Phase("build_plan");
	const Plan &P = plan;
	const int64_t n_lblocks = int64_t(P.lrow.size());
	const SparseRecordOptions t_opt = t_Record_Options(*this, b_timing);
	const bool b_small = t_opt.b_small;
	lists.n_bottom_stages = count_bottom_stages(P, t_opt);
	SparseRecords rec; // (declared ahead of the threads that fill and read it: they are joined before it goes)

	// 2. the shape grouping of the leaf kernel (13 ms of host work at 100 000 poses, plan in, tables out) runs beside the
	// records, packages and uploads below
	std::exception_ptr p_simt_error;
	CJoinedThread t_simt_thread;
	const double t_simt = wall_ms();
	if(b_small)
		build_simt_tables(P, t_opt, rec, lists);
	else {
		t_simt_thread.t = std::thread([&]() {
			try {
				build_simt_tables(P, t_opt, rec, lists);
			} catch(...) {
				p_simt_error = std::current_exception();
			}
		});
	}

	// 3. Round 6: the columns of the separator stages first (a tenth of the records at C3) -- the packages of their tasks, the longest
	// single-threaded piece of the analysis, are built from those on a thread of their own while this one writes the rest
	alloc_column_records(P, rec);
	const int64_t n_upper_begin = first_upper_column(P, t_opt, lists), n_sched = int64_t(rec.cols.size());
	fill_column_records(P, rec, n_upper_begin, n_sched);
	reserve_panel_packages(P, lists, n_upper_begin, rec);

	// 4. the panel packages of the separator stages
	std::exception_ptr p_panel_error;
	CJoinedThread t_panel_thread;
	if(b_small)
		build_panel_packages(P, t_opt, rec, lists);
	else {
		t_panel_thread.t = std::thread([&]() {
			try {
				const double t_panel = wall_ms();
				build_panel_packages(P, t_opt, rec, lists);
				if(b_timing)
					fprintf(stderr, "[setup] %-12s %8.2f ms on their own thread\n", "panel pkgs", wall_ms() - t_panel);
			} catch(...) {
				p_panel_error = std::current_exception();
			}
		});
	}

	// 5. the remaining records
	Parallel_Ranges(n_upper_begin, 4096, [&](int64_t i_begin, int64_t i_end) { fill_column_records(P, rec, i_begin, i_end); }, 8);
	fill_dense_top_column_records(P, rec);

	// 6. column packages of the upper stages
	build_column_packages(P, lists, rec);
	Phase("records");

	// 7. the records go to the device beside the host work that follows (the packages of the separator tasks: ~10 ms each at C3,
	// and an upload from a std::vector is a staged copy that keeps its thread): a thread of its own, joined before the rest
	// of the uploads.  The vectors it reads are not written from here on.
	std::exception_ptr p_upload_error;
	CJoinedThread t_upload_thread;
	if(b_small) {
		Upload_Records(*this, rec);
		Phase("record uploads");
	} else {
		t_upload_thread.t = std::thread([&]() {
			try {
				Upload_Records(*this, rec);
			} catch(...) {
				p_upload_error = std::current_exception();
			}
		});
	}
	Join_Bringup(); // (this thread's own uploads and allocations begin below)

	// 8. dense top
	n_dense_dim = P.dense_dim;
	n_dense_pad = n_dense_dim? dense_padded_dim(n_dense_dim) : 0;
	build_dense_top_records(P, n_dense_pad, rec);
	if(n_dense_dim)
		Setup_Dense_Top(*this, rec, Phase);
	n_dense_blks = int(rec.dense_blks.size());
	n_dense_cols = int(rec.dense_cols.size());
	Phase("tile schedule");

	// 9. join, uploads, allocations
	if(t_panel_thread.t.joinable())
		t_panel_thread.t.join();
	if(p_panel_error)
		std::rethrow_exception(p_panel_error);
	Phase("packages");
	d_panel_upd_slots.Upload(rec.upd_slots, stream);
	d_panel_upd_ents.Upload(rec.upd_ents, stream);
	d_panel_pkg.Upload(rec.panel_pkg, stream);
	d_panel_off.Upload(rec.panel_off, stream);
	d_panel_out_off.Upload(rec.panel_out_off, stream);
	d_handup.Alloc(size_t(std::max<int64_t>(rec.n_handup_doubles, int64_t(P.max_dim) * P.max_dim + 8))); // (every wave of a fused panel launch prefetches one block + 8 from offset 0, hand-ups or not)
	d_panel_rest.Upload(rec.panel_rest, stream);
	n_lds_limit = plain_launch_lds_limit();
	d_bwd_rec.Upload(rec.bwd_rec, stream);
	d_bwd_off.Upload(rec.bwd_off, stream);
	if(t_upload_thread.t.joinable())
		t_upload_thread.t.join();
	if(p_upload_error)
		std::rethrow_exception(p_upload_error);
	Phase("uploads");
	d_L.Alloc(size_t(P.loff[n_lblocks]));
	d_Linv.Alloc(size_t(P.linv_off[P.n]));
	d_w.Alloc(size_t(P.cs_new[P.n]));
	d_flag.Alloc(1);
	SLAMPP_HIP_CHECK(hipMemsetAsync(d_flag.p(), 0, sizeof(int), stream)); // sync() before the first factorization reads it
	Phase("allocs");
	SLAMPP_HIP_CHECK(hipStreamSynchronize(stream)); // (every copy above has left its host array)
	Phase("sync");

	// 10. the device's view of the plan
	dplan.cols = d_cols.p(); dplan.blks = d_blks.p(); dplan.pairs = d_pairs.p(); dplan.rents = d_rents.p();
	dplan.task_ptr = d_task_ptr.p();
	dplan.uniform_dim = P.uniform_dim? P.max_dim : 0;
	dplan.pkg = d_pkg.p();
	dplan.task_pkg = d_pkg.p()? d_task_pkg.p() : 0;
	dplan.n_blks = n_lblocks;
	dplan.n_pairs = int64_t(rec.pairs.size());
	dplan.n_rents = int64_t(rec.rents.size());
	dplan.p_timing = 0;
	dplan.task_map = 0;
	{
		const double t_wait = wall_ms();
		if(t_simt_thread.t.joinable())
			t_simt_thread.t.join();
		if(p_simt_error)
			std::rethrow_exception(p_simt_error);
		Upload_Simt(rec);
		if(b_timing)
			fprintf(stderr, "[setup] %-12s %8.2f ms since it was started, %.2f ms of them waited for\n", "shapes", wall_ms() - t_simt, wall_ms() - t_wait);
	}
	if(getenv("SLAMPP_HIP_STAGE_TIMING")) { // development aid: clock samples of the upper-stage kernel, printed at sync
		d_timing.Alloc(1 + 32 * 4096);
		SLAMPP_HIP_CHECK(hipMemsetAsync(d_timing.p(), 0, (1 + 32 * 4096) * sizeof(long long), stream));
		dplan.p_timing = d_timing.p();
	}

	// 11. discard
	if(!b_small) {
		// the record vectors are on the device: giving their memory back to the system (70 MB at C3: 3 - 4 ms of page-table
		// work) is nobody's critical path -- a thread does it behind the analysis' return (host_pool.h: TTrash, t_discard)
		Join_Discard();
		Discard_Later(analysis_trash, rec.cols); Discard_Later(analysis_trash, rec.blks); Discard_Later(analysis_trash, rec.pairs);
		Discard_Later(analysis_trash, rec.rents); Discard_Later(analysis_trash, rec.pkg); Discard_Later(analysis_trash, rec.task_pkg);
		Discard_Later(analysis_trash, rec.panel_pkg); Discard_Later(analysis_trash, rec.upd_slots); Discard_Later(analysis_trash, rec.upd_ents);
		Discard_Later(analysis_trash, rec.simt_tab); Discard_Later(analysis_trash, rec.simt_bwd_tab);
		try {
			t_discard = std::thread([this]() { analysis_trash.clear(); host_pool_release(); });
		} catch(std::system_error&) {
			analysis_trash.clear();
			host_pool_release();
		}
	}
}

// inv(L_jj) of the columns of the lane-per-task stages, where the factorization left them out: computed from the factor, once
// per factorization, and stored by every factorization from now on
void slampp_hip_solver::Ensure_Leaf_Inverses()
{
	b_leaf_linv_wanted = true;
	if(b_leaf_linv_valid || lists.simt_chunk_ptr.empty())
		return;
	const Plan &P = plan;
	const int n_simt_stages_used = int(lists.simt_chunk_ptr.size()) - 1;
	const int64_t n_col_end = P.task_ptr[size_t(P.stage_ptr[size_t(n_simt_stages_used)])];
	launch_invert_diagonals(dplan, 0, n_col_end, d_L.p(), d_Linv.p(), stream);
	b_leaf_linv_valid = true;
}

// development print (SLAMPP_HIP_PLAN_TIMING): what the column loop of the lane-per-task backward kernels meets, per stage, counted in tasks
// (the spare lanes of a chunk repeat its last task: not counted)
void slampp_hip_solver::Report_Simt_Backward(const SparseRecords &r_rec) const
{
	enum { N_MAX = 16 }; // (the last bin collects everything beyond)
	for(size_t s = 0; s + 1 < lists.simt_chunk_ptr.size(); ++ s) {
		long long n_by_cols[N_MAX + 1] = {0}, n_by_blocks[N_MAX + 1] = {0}, n_by_outside[SIMT_BWD_AHEAD + 1] = {0}, n_inside = 0, n_outside = 0, n_tasks = 0;
		int n_spare_chunks = 0;
		for(int32_t c = lists.simt_chunk_ptr[s]; c < lists.simt_chunk_ptr[s + 1]; ++ c) {
			const TSimtChunk &ch = r_rec.simt_bwd_chunks[size_t(c)];
			const int32_t *P = &r_rec.simt_bwd_prog[size_t(ch.prog_off)]; // n_cols, blocks below the diagonals, nb per column, the rows' places
			const int n_cols = P[0], n_below = P[1];
			n_tasks += ch.n_tasks;
			n_spare_chunks += ch.n_tasks < n_simt_width;
			n_by_cols[std::min(n_cols, int(N_MAX))] += ch.n_tasks;
			for(int i = 0, n_blk0 = 0; i < n_cols; n_blk0 += P[2 + i] - 1, ++ i) {
				n_by_blocks[std::min(P[2 + i] - 1, int(N_MAX))] += ch.n_tasks;
				int n_set_outside = 0; // rows outside the task among the blocks a register set of the fetch-ahead form holds
				for(int k = 0; k < SIMT_BWD_AHEAD && k < P[2 + i] - 1; ++ k)
					n_set_outside += P[2 + n_cols + n_blk0 + k] < 0;
				n_by_outside[n_set_outside] += ch.n_tasks;
			}
			for(int b = 0; b < n_below; ++ b)
				((P[2 + n_cols + b] >= 0)? n_inside : n_outside) += ch.n_tasks;
		}
		std::string s_cols, s_blocks, s_outside;
		for(int i = 0; i <= SIMT_BWD_AHEAD; ++ i)
			s_outside += " " + std::to_string(i) + ":" + std::to_string(n_by_outside[i]);
		for(int i = 0; i <= N_MAX; ++ i) {
			if(n_by_cols[i])
				s_cols += " " + std::to_string(i) + ":" + std::to_string(n_by_cols[i]);
			if(n_by_blocks[i])
				s_blocks += " " + std::to_string(i) + ":" + std::to_string(n_by_blocks[i]);
		}
		fprintf(stderr, "[setup] stage %zu backward lanes: %lld tasks in %d chunks of width %d, %d chunks with spare lanes, fetch ahead holds %d blocks, one round holds %d waves; "
			"tasks by columns:%s; columns by sub-diagonal blocks:%s; columns by rows outside the task among the blocks held:%s; blocks with the row inside the task: %lld, outside: %lld\n", s, n_tasks,
			lists.simt_chunk_ptr[s + 1] - lists.simt_chunk_ptr[s], n_simt_width, n_spare_chunks, int(SIMT_BWD_AHEAD),
			(s < simt_bwd_ahead_waves.size())? simt_bwd_ahead_waves[s] : 0, s_cols.c_str(), s_blocks.c_str(), s_outside.c_str(), n_inside, n_outside);
	}
}

// development print (SLAMPP_HIP_PLAN_TIMING): what the column loop of the lane-per-task factor kernels meets, per stage, counted in tasks
// (the spare lanes of a chunk repeat its last task: not counted).  A block below the diagonal either has a source in Lambda or is
// fill-in (enc < 0 in the task's table: tasks of one shape may differ in it)
void slampp_hip_solver::Report_Simt_Factor(const SparseRecords &r_rec) const
{
	enum { N_MAX = 16 }; // (the last bin collects everything beyond)
	for(size_t s = 0; s + 1 < lists.simt_chunk_ptr.size(); ++ s) {
		long long n_by_cols[N_MAX + 1] = {0}, n_by_blocks[N_MAX + 1] = {0}, n_by_sources[N_MAX + 1] = {0}, n_by_fill[N_MAX + 1] = {0}, n_held_fill = 0, n_tasks = 0;
		int n_spare_chunks = 0;
		for(int32_t c = lists.simt_chunk_ptr[s]; c < lists.simt_chunk_ptr[s + 1]; ++ c) {
			const TSimtChunk &ch = r_rec.simt_chunks[size_t(c)];
			const int32_t *P = &r_rec.simt_prog[size_t(ch.prog_off)]; // n_cols, n_blocks, n_ops, n_y, then the columns
			const int64_t *T = &r_rec.simt_tab[size_t(ch.tab_off)]; // [field][width]
			const int n_cols = P[0];
			n_tasks += ch.n_tasks;
			n_spare_chunks += ch.n_tasks < n_simt_width;
			n_by_cols[std::min(n_cols, int(N_MAX))] += ch.n_tasks;
			for(int i = 0, pc = 4, n_blk0 = 0; i < n_cols; ++ i) {
				const int nb = P[pc], nr = P[pc + 1], n_touch = P[pc + 2];
				pc += 3 + n_touch + 2 * nr;
				for(int kb = 1; kb < nb; ++ kb)
					pc += 1 + 2 * P[pc];
				n_by_blocks[std::min(nb - 1, int(N_MAX))] += ch.n_tasks;
				for(int t = 0; t < ch.n_tasks; ++ t) {
					int n_sources = 0, n_fill = 0;
					for(int kb = 1; kb < nb; ++ kb) {
						const bool b_fill = T[size_t(4 * n_cols + n_blk0 + kb) * size_t(n_simt_width) + size_t(t)] < 0;
						(b_fill? n_fill : n_sources) ++;
						n_held_fill += b_fill && kb <= int(SIMT_FACTOR_AHEAD);
					}
					n_by_sources[std::min(n_sources, int(N_MAX))] ++;
					n_by_fill[std::min(n_fill, int(N_MAX))] ++;
				}
				n_blk0 += nb;
			}
		}
		std::string s_cols, s_blocks, s_sources, s_fill;
		for(int i = 0; i <= N_MAX; ++ i) {
			if(n_by_cols[i])
				s_cols += " " + std::to_string(i) + ":" + std::to_string(n_by_cols[i]);
			if(n_by_blocks[i])
				s_blocks += " " + std::to_string(i) + ":" + std::to_string(n_by_blocks[i]);
			if(n_by_sources[i])
				s_sources += " " + std::to_string(i) + ":" + std::to_string(n_by_sources[i]);
			if(n_by_fill[i])
				s_fill += " " + std::to_string(i) + ":" + std::to_string(n_by_fill[i]);
		}
		fprintf(stderr, "[setup] stage %zu factor lanes: %lld tasks in %d chunks of width %d, %d chunks with spare lanes, fetch ahead holds %d blocks, one round holds %d waves; "
			"tasks by columns:%s; columns by sub-diagonal blocks:%s; columns by sub-diagonal blocks with a source in Lambda:%s; columns by fill-in blocks:%s; "
			"fill-in blocks among the blocks held: %lld\n", s, n_tasks, lists.simt_chunk_ptr[s + 1] - lists.simt_chunk_ptr[s], n_simt_width, n_spare_chunks,
			int(SIMT_FACTOR_AHEAD), (s < simt_factor_ahead_waves.size())? simt_factor_ahead_waves[s] : 0, s_cols.c_str(), s_blocks.c_str(), s_sources.c_str(),
			s_fill.c_str(), n_held_fill);
	}
}

// the lane-per-task tables build_simt_tables() made
void slampp_hip_solver::Upload_Simt(const SparseRecords &r_rec)
{
	const Plan &P = plan;
	if(r_rec.simt_chunks.empty())
		return;
	d_simt_chunks.Upload(r_rec.simt_chunks, stream);
	d_simt_prog.Upload(r_rec.simt_prog, stream);
	d_simt_tab.Upload(r_rec.simt_tab, stream);
	d_simt_rest.Upload(r_rec.simt_rest, stream);
	d_simt_bwd_chunks.Upload(r_rec.simt_bwd_chunks, stream);
	d_simt_bwd_prog.Upload(r_rec.simt_bwd_prog, stream);
	d_simt_bwd_tab.Upload(r_rec.simt_bwd_tab, stream);
	d_simt_br_groups.Upload(r_rec.simt_br_groups, stream);
	d_simt_bwd_br_groups.Upload(r_rec.simt_bwd_br_groups, stream);
	SLAMPP_HIP_CHECK(hipStreamSynchronize(stream)); // (the host copies are no longer needed)
	simt_branches_round_groups.clear();
	for(size_t s = 0; s < lists.simt_br.size(); ++ s)
		simt_branches_round_groups.push_back((lists.simt_br[s].n_groups > 0)? factor_simt_branches_groups(P.max_dim, n_simt_width, lists.simt_br[s].n_lds_bytes) : 0);
	simt_bwd_branches_round_groups.clear();
	for(size_t s = 0; s < lists.simt_br.size(); ++ s)
		simt_bwd_branches_round_groups.push_back((lists.simt_br[s].n_bwd_groups > 0)? backward_simt_branches_groups(P.max_dim, n_simt_width, lists.simt_br[s].n_bwd_lds_bytes) : 0);
	simt_bwd_ahead_waves.clear();
	for(size_t s = 0; s < lists.simt_bwd_lds_bytes.size(); ++ s)
		simt_bwd_ahead_waves.push_back(backward_simt_ahead_waves(P.max_dim, n_simt_width, lists.simt_bwd_lds_bytes[s]));
	simt_factor_ahead_waves.clear();
	for(size_t s = 0; s < lists.simt_lds_bytes.size(); ++ s)
		simt_factor_ahead_waves.push_back(factor_simt_ahead_waves(P.max_dim, n_simt_width, lists.simt_lds_bytes[s]));
	if(getenv("SLAMPP_HIP_PLAN_TIMING")) {
		Report_Simt_Backward(r_rec);
		Report_Simt_Factor(r_rec);
		for(size_t s = 0; s < lists.simt_br.size(); ++ s) { // the two-wave form's records (sparse_records.cpp: Build_Simt_Branches())
			const TSimtBranchStage &r_br = lists.simt_br[s];
			if(!r_br.n_groups)
				continue;
			std::string s_by;
			for(size_t i = 0; i + 2 < r_br.split_by.size(); i += 3)
				s_by += " (" + std::to_string(r_br.split_by[i]) + "," + std::to_string(r_br.split_by[i + 1]) + "):" + std::to_string(r_br.split_by[i + 2]);
			fprintf(stderr, "[setup] stage %zu factor branches: %d split tasks in %d split chunks, %d whole chunks, %d workgroups of two waves, T* %d, longest chain %d, "
				"longest task %d; split tasks by (longer bin, join columns):%s; LDS %d bytes, one round holds %d workgroups\n", s, r_br.n_split_tasks, r_br.n_split_chunks,
				r_br.n_whole_chunks, r_br.n_groups, r_br.n_tstar, r_br.n_longest_chain, r_br.n_longest_task, s_by.c_str(), r_br.n_lds_bytes,
				(s < simt_branches_round_groups.size())? simt_branches_round_groups[s] : 0);
			if(!r_br.n_bwd_groups)
				continue;
			fprintf(stderr, "[setup] stage %zu backward branches: %d split tasks in %d split chunks, %d whole chunks, %d workgroups of two waves, width %d, T* %d, longest chain %d, "
				"longest task %d; split tasks by (longer bin, join columns):%s; split tasks with three tips or more: %d; segment columns with more than %d blocks: %d; "
				"columns with two rows outside the task or more: %d; chunks with spare lanes: %d; LDS %d bytes (three table regions of %d entries, two x regions of %d doubles), "
				"one round holds %d workgroups\n", s, r_br.n_split_tasks, r_br.n_split_chunks, r_br.n_whole_chunks, r_br.n_bwd_groups, n_simt_width, r_br.n_tstar, r_br.n_longest_chain,
				r_br.n_longest_task, s_by.c_str(), r_br.n_bwd_tip3_tasks, int(SIMT_BWD_AHEAD) + 1, r_br.n_bwd_long_columns, r_br.n_bwd_two_outside_columns, r_br.n_bwd_spare_chunks,
				r_br.n_bwd_lds_bytes, r_br.n_bwd_tab_region, r_br.n_bwd_x_region, (s < simt_bwd_branches_round_groups.size())? simt_bwd_branches_round_groups[s] : 0);
		}
		for(size_t s = 0; s + 1 < lists.simt_chunk_ptr.size(); ++ s) {
			fprintf(stderr, "[setup] stage %zu: %d tasks -> %d chunks of 64 lanes, %d tasks left to the wave-per-task kernel\n", s,
				P.stage_ptr[s + 1] - P.stage_ptr[s], lists.simt_chunk_ptr[s + 1] - lists.simt_chunk_ptr[s], lists.simt_rest_ptr[s + 1] - lists.simt_rest_ptr[s]);
		}
	}
}
