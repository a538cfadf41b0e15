// sparse_records.h -- host records of the sparse block path: what the analysis lays out for the kernels (sparse_kernels.h),
// from the plan alone.  Host code only: no HIP call, nothing of the handle (solver.h); sparse_setup.hip runs these builders
// on its threads and uploads what they made, tests/sparse_records_driver.cpp runs them on the CPU under sanitizers.
#pragma once
#include "plan.h"
#include "sparse_kernels.h"
#include "host_pool.h"
#include "host_threads.h"

#include <algorithm>

namespace slampp {

// what the builders read of the handle's options (filled by sparse_setup.hip); the development knobs (plan.h) are read
// by the builders themselves, where they apply
struct SparseRecordOptions {
	int n_panel;          // option "panel"
	int n_panel_handup;   // option "panel_handup"
	int n_simt;           // option "simt"
	int n_simt_width;     // option "simt_width"
	int n_simt_stages;    // option "simt_stages"
	int n_wide_min_tasks; // option "wide_min_tasks"
	bool b_small;         // a small system: all host work on the calling thread
	bool b_timing;        // SLAMPP_HIP_PLAN_TIMING: the builders print what they decided
};

// a lane-per-task stage's workgroup records of the two-wave factor form (sparse_kernels.h: TSimtBranchGroup)
struct TSimtBranchStage {
	int32_t n_first = 0, n_groups = 0;  // the stage's records in SparseRecords::simt_br_groups (none: the stage keeps the one-wave forms)
	int32_t n_split_tasks = 0, n_split_chunks = 0, n_whole_chunks = 0;
	int32_t n_tstar = 0;                // T*: the largest, over the stage's shapes, of min(columns, chain)
	int32_t n_longest_chain = 0;        // the longest chain of columns a wave walks with these records
	int32_t n_longest_task = 0, n_stage_tasks = 0;
	int32_t n_lds_bytes = 0;            // two regions of the largest segment table
	std::vector<int32_t> split_by;      // triples: longer bin, join columns, tasks
	// the same items in the same order as backward records (sparse_kernels.h: TSimtBwdBranchLaunch), in SparseRecords::simt_bwd_br_groups
	int32_t n_bwd_first = 0, n_bwd_groups = 0; // (none: the LDS request is beyond a plain launch's, the stage keeps the one-wave backward forms)
	int32_t n_bwd_tab_region = 0, n_bwd_x_region = 0, n_bwd_lds_bytes = 0; // entries, doubles, (3 tab + 2 x) * 8
	// what the column loop meets in these records, for the report (SLAMPP_HIP_PLAN_TIMING): split tasks with three or more tips;
	// columns of split tasks' segments with more blocks than a register set holds; columns of the records with two or more rows
	// outside the task among the blocks held; chunks with spare lanes
	int32_t n_bwd_tip3_tasks = 0, n_bwd_long_columns = 0, n_bwd_two_outside_columns = 0, n_bwd_spare_chunks = 0;
};

// what the launches of a step read on the host (sparse_enqueue.hip)
struct SparseLaunchLists {
	int n_bottom_stages = 1; // leading stages launched with one wave per task
	// separator tasks that run as panels in LDS (panel_kernel.hip)
	std::vector<int32_t> panel_ptr, panel_rest_ptr, panel_upd_ptr; // [n_stages + 1] ranges of the lists (empty: no panels)
	std::vector<TPanelLaunch> panel_cfg; // [n_stages] waves per task and LDS capacities of the stage's panel launch
	std::vector<TBwdLaunch> bwd_cfg;     // [n_stages] the shape of the stage's backward launch (backward_slice_kernel)
	std::vector<char> panel_ride; // [n_stages + 1] the stage's updates from further down are applied inside the launch of the stage below (2: the tasks bring in everything themselves)
	bool b_any_hand_up = false;
	// lane-per-task kernels of the wide bottom stages (simt_kernel.hip)
	std::vector<int32_t> simt_chunk_ptr, simt_rest_ptr; // [n_bottom_stages + 1] each; empty = not in use
	std::vector<int32_t> simt_lds_bytes, simt_bwd_lds_bytes; // per stage: the largest chunk table (it is staged in LDS)
	std::vector<TSimtBranchStage> simt_br; // per stage (empty: no stage has records)
};

// the host arrays of one analysis, until they are on the device
struct SparseRecords {
	// packed device records (see sparse_kernels.h)
	raw_vector<TColDesc> cols; // in schedule order (raw_vector: not zero-filled -- host_pool.h; every record is written in full)
	raw_vector<TBlkDesc> blks;
	raw_vector<longlong2> pairs;
	raw_vector<TRowEnt> rents;
	// column packages of the upper stages
	raw_vector<longlong2> pkg;
	std::vector<int64_t> task_pkg;
	// panel packages of the separator stages, and the updates those tasks receive from earlier stages (panel_update_kernel)
	raw_vector<longlong2> panel_pkg; // (raw_vector: the big arrays of the analysis live in mappings of the library's own, on huge pages)
	std::vector<int64_t> panel_off, panel_out_off; // (panel_out_off: per package the offset of its hand-up list, or -1)
	std::vector<int32_t> panel_units; // per package its size in 16-byte units: what the launch order of a stage goes by
	std::vector<int32_t> panel_rest;  // the tasks of the panel stages left to the column kernel
	raw_vector<longlong2> bwd_rec;    // backward records of the packaged tasks (TBwdHead ..)
	std::vector<int64_t> bwd_off;     // per package (as panel_off) the offset of its backward record | its units << BWD_OFF_BITS
	raw_vector<TUpdSlot> upd_slots;
	raw_vector<TUpdEnt> upd_ents;
	int64_t n_handup_doubles = 0;
	// dense top
	std::vector<TDenseBlk> dense_blks;
	std::vector<TDenseCol> dense_cols;
	std::vector<int64_t> dense_blk_loff;
	std::vector<int32_t> gaps;   // positions inside the dense top that no column maps to
	std::vector<uint8_t> unit;   // per position of the padded dense top: 1 = padding or gap
	std::vector<longlong2> dst;  // per position: where x goes (.x in the workspace, .y in the caller's vector; < 0: nowhere)
	// lane-per-task tables, forward and backward
	std::vector<TSimtChunk> simt_chunks, simt_bwd_chunks;
	std::vector<int32_t> simt_prog, simt_rest, simt_bwd_prog;
	raw_vector<int64_t> simt_tab, simt_bwd_tab; // (raw_vector: written in full by the table pass, never zero-filled)
	std::vector<TSimtBranchGroup> simt_br_groups; // (the segments' programs and tables lie behind the chunks' in simt_prog and simt_tab)
	std::vector<TSimtBranchGroup> simt_bwd_br_groups; // the same records of backward chunks (programs and tables behind the chunks' in simt_bwd_prog and simt_bwd_tab)
};

// index ranges on a few threads (the record loops of the cold path: every entry written once, from the plan alone)
template <class F>
void Parallel_Ranges(int64_t n, int64_t n_min_per_thread, F f, int n_max_threads = 4)
{
	for_ranges(0, n, host_thread_count(n, n_min_per_thread, n_max_threads), [&](int, int64_t n_b, int64_t n_e) { f(n_b, n_e); });
}

// The builders, one per job.  Each reads the plan, the options and what earlier builders left, and writes the parts named;
// all throw (std::domain_error: a system the sparse path does not take).

// the bottom stage and the wide stages right above it, which run one wave per task
int count_bottom_stages(const Plan &P, const SparseRecordOptions &t_opt);
// where the columns of the separator stages begin in the schedule (their records are written first: the panel packages are
// built from them beside the rest); 0 where the leaf tasks may get panel packages too
int64_t first_upper_column(const Plan &P, const SparseRecordOptions &t_opt, const SparseLaunchLists &r_lists);
// sizes cols, blks, pairs, rents (not filled)
void alloc_column_records(const Plan &P, SparseRecords &r_rec);
// everything of the scheduled columns [i_begin, i_end): their records, their blocks, those blocks' update pairs, the row
// entries of their diagonal blocks.  Ranges may be filled in any order and side by side.
void fill_column_records(const Plan &P, SparseRecords &r_rec, int64_t i_begin, int64_t i_end);
// the blocks, pairs and row entries of the dense top's columns (not scheduled; their records are read all the same)
void fill_dense_top_column_records(const Plan &P, SparseRecords &r_rec);
// address space for the panel lists up front (reads cols[n_upper_begin ..))
void reserve_panel_packages(const Plan &P, const SparseLaunchLists &r_lists, int64_t n_upper_begin, SparseRecords &r_rec);
// panel_pkg .. n_handup_doubles, and the panel_* members of the launch lists; reads cols, blks, rents of the columns from
// n_upper_begin on (see first_upper_column) and n_bottom_stages
void build_panel_packages(const Plan &P, const SparseRecordOptions &t_opt, SparseRecords &r_rec, SparseLaunchLists &r_lists);
// pkg, task_pkg; reads cols, blks, pairs, rents and n_bottom_stages
void build_column_packages(const Plan &P, const SparseLaunchLists &r_lists, SparseRecords &r_rec);
// dense_blks .. dst; n_dense_pad: the padded dimension of the dense system
void build_dense_top_records(const Plan &P, int n_dense_pad, SparseRecords &r_rec);
// The segments of a leaf task for the two-wave factor form, from the parents of its columns inside the task (-1: none; columns
// in elimination order, a parent behind its children).  Join columns: those with two or more children inside the task, and
// their ancestors.  The others fall into chains, each from a tip up to just below the first join column; the chains go into two
// bins, longest first, each into the currently shorter bin (ties: the first).  seg[0], seg[1]: the bins, seg[2]: the join
// columns, all ascending.  A task with one tip has one bin and no joins.  Returns the task's chain: the longer bin plus the joins.
struct TSimtSegments {
	std::vector<int32_t> seg[3];
	int32_t n_tips = 0;
};
void simt_task_parents(const Plan &P, int32_t t, std::vector<int32_t> &r_parent);
int32_t simt_task_segments(const std::vector<int32_t> &r_parent, TSimtSegments &r_seg);
// simt_* of both; reads n_bottom_stages
void build_simt_tables(const Plan &P, const SparseRecordOptions &t_opt, SparseRecords &r_rec, SparseLaunchLists &r_lists);

} // namespace slampp
