// sparse_records.cpp -- the host records of the sparse block path (sparse_records.h): column records, column packages,
// panel packages with their hand-up lists, dense-top records, lane-per-task tables.  Host code only.
#include "sparse_records.h"

#include <climits>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <map>
#include <stdexcept>
#include <unordered_map>

namespace slampp {

static bool b_Package_Dim(const Plan &P) // the block sizes the package kernels are built for
{
	return P.uniform_dim && (P.max_dim == 3 || P.max_dim == 6 || P.max_dim == 7);
}

int count_bottom_stages(const Plan &P, const SparseRecordOptions &t_opt)
{
	// the bottom stage and the wide stages right above it (more tasks than the 8-wave kernel keeps
	// resident at 2 workgroups per CU) run one wave per task: there throughput beats single-column latency
	int n_bottom_stages = 1;
	while(n_bottom_stages < int(P.stage_ptr.size()) - 1 &&
	   P.stage_ptr[n_bottom_stages + 1] - P.stage_ptr[n_bottom_stages] > t_opt.n_wide_min_tasks)
		++ n_bottom_stages; // (tall tasks, Plan::col_sub, begin above these: the same threshold)
	return n_bottom_stages;
}

int64_t first_upper_column(const Plan &P, const SparseRecordOptions &t_opt, const SparseLaunchLists &r_lists)
{
	return (t_opt.b_small || P.stage_ptr.size() < 2 || P.stage_ptr[1] - P.stage_ptr[0] <= 512)? 0 : // (few leaf tasks: they may get panel packages too)
		 P.task_ptr[size_t(P.stage_ptr[size_t(std::min(r_lists.n_bottom_stages, int(P.stage_ptr.size()) - 1))])];
}

void alloc_column_records(const Plan &P, SparseRecords &r_rec)
{
	if(P.cs_new[P.n] >= INT32_MAX)
		throw std::domain_error("systems with 2^31 or more scalar unknowns are not supported by the sparse path");
	const int64_t n_lblocks = int64_t(P.lrow.size());
	r_rec.cols.resize(P.task_cols.size()); // all columns but those of the dense top
	r_rec.blks.resize(size_t(n_lblocks));
	r_rec.pairs.resize(P.pa.size());
	r_rec.rents.resize(P.rblk.size());
	if(P.loff[n_lblocks] >= (int64_t(1) << 48))
		throw std::domain_error("the factor has 2^48 or more values");
}

// everything of one column: its blocks, their update pairs (stored block by block), the row entries of its diagonal block
static void Fill_Column(const Plan &P, SparseRecords &r_rec, int32_t j)
{
	for(int64_t k = P.lptr[j]; k < P.lptr[j + 1]; ++ k) {
		TBlkDesc &b = r_rec.blks[k];
		const int64_t np = P.pptr[k + 1] - P.pptr[k];
		if(np >= (int64_t(1) << 24))
			throw std::domain_error("a factor block has 2^24 or more updates: use the dense path");
		b.loff = P.loff[k];
		b.asrc = (P.asrc[k] < 0)? -1 : P.asrc[k] * 2 + P.atrans[k];
		if(k == P.lptr[j] && b.asrc >= 0)
			b.asrc |= 1; // diagonal blocks are read transposed: the lower triangle of the factor block then comes from the upper triangle of Lambda's block, the one the reference's solvers consume
		b.p0 = P.pptr[k];
		b.np_di = uint32_t(np) | (uint32_t(P.dim[P.lrow[k]]) << 24);
		b.xcs = int32_t(P.cs_new[P.lrow[k]]);
		const int64_t n_pos = std::min<int64_t>(k - P.lptr[j], 255); // position of the target block in its column
		for(int64_t e = P.pptr[k]; e < P.pptr[k + 1]; ++ e) {
			const int64_t dc = P.dim[P.blk_col[P.pa[e]]];
			r_rec.pairs[e].x = P.loff[P.pa[e]] | (n_pos << 48) | (dc << 56);
			r_rec.pairs[e].y = P.loff[P.pb[e]];
		}
	}
	for(int64_t e = P.rptr[j]; e < P.rptr[j + 1]; ++ e) {
		const int32_t c = P.blk_col[P.rblk[e]];
		r_rec.rents[e].off = P.loff[P.rblk[e]];
		r_rec.rents[e].ycs = int32_t(P.cs_new[c]);
		r_rec.rents[e].dc = P.dim[c];
	}
}

void fill_column_records(const Plan &P, SparseRecords &r_rec, int64_t i_begin, int64_t i_end)
{
	for(int64_t i = i_begin; i < i_end; ++ i) {
		const int32_t j = P.task_cols[i];
		TColDesc &c = r_rec.cols[i];
		memset(&c, 0, sizeof(c));
		c.k0 = P.lptr[j];
		c.nb = int32_t(P.lptr[j + 1] - P.lptr[j]);
		c.dj = P.dim[j];
		c.linv_off = P.linv_off[j];
		c.cs_new = P.cs_new[j];
		c.cs_src = P.cs_src[j];
		c.r0 = P.rptr[j];
		c.nr = int32_t(P.rptr[j + 1] - P.rptr[j]);
		c.p0 = P.pptr[P.lptr[j] + 1]; // pairs are stored block by block: those of the sub-diagonal blocks are contiguous
		const int64_t np = P.pptr[P.lptr[j + 1]] - c.p0;
		c.np = int32_t(std::min<int64_t>(np, INT32_MAX));
		Fill_Column(P, r_rec, j);
	}
}

void fill_dense_top_column_records(const Plan &P, SparseRecords &r_rec)
{
	for(int32_t j = 0; j < P.n; ++ j) {
		if(P.dense_pos[j] >= 0)
			Fill_Column(P, r_rec, j);
	}
}

void reserve_panel_packages(const Plan &P, const SparseLaunchLists &r_lists, int64_t n_upper_begin, SparseRecords &r_rec)
{
	// room for everything up front (address space only: pages come when they are written): the lists used to grow by
	// doubling, each step an mmap, a copy and a munmap of megabytes -- and a munmap interrupts every thread of the process
	// (the TLB shootdown), of which the analysis runs a dozen at this point (round 6)
	const size_t n_upper_tasks = (P.stage_ptr.size() > 1)? size_t(P.stage_ptr.back() - P.stage_ptr[size_t(std::min(r_lists.n_bottom_stages, int(P.stage_ptr.size()) - 1))]) : 0;
	const size_t n_tasks_cap = (n_upper_begin == 0)? P.task_ptr.size() : n_upper_tasks;
	size_t n_upper_blocks = 0, n_upper_pairs = 0;
	for(int64_t i = n_upper_begin; i < int64_t(r_rec.cols.size()); ++ i) {
		n_upper_blocks += size_t(r_rec.cols[i].nb);
		n_upper_pairs += size_t(r_rec.cols[i].np) + size_t(r_rec.cols[i].nr);
	}
	r_rec.panel_pkg.reserve(n_tasks_cap * 64 + 3 * n_upper_blocks + n_upper_pairs + 64 * PANEL_W + 4096);
	r_rec.upd_slots.reserve(n_upper_blocks + 16);
	r_rec.upd_ents.reserve(n_upper_pairs + 16);
	r_rec.panel_off.reserve(n_tasks_cap + 16);
	r_rec.panel_out_off.reserve(n_tasks_cap + 16);
	r_rec.bwd_rec.reserve(n_tasks_cap * (4 + 2 * PANEL_COLS) + n_upper_blocks + 16);
	r_rec.bwd_off.reserve(n_tasks_cap + 16);
}

// ---- panel packages for the separator stages (panel_kernel.hip) ----
// A task qualifies if its columns' blocks are one range of the factor and everything fits the kernel's LDS; the updates it
// receives from earlier stages go to the lists of panel_update_kernel, block by block.

namespace {

static_assert(sizeof(TBwdHead) == 64 && sizeof(TBwdCol) == 32 && sizeof(TBwdBlk) == 16, "record sizes");
static_assert(sizeof(TPanelOut) == 16 && sizeof(TPanelHead) == 64 && sizeof(TPanelCol) == 48 && sizeof(TPanelSlot) == 32 && sizeof(TPanelExt) == 32 && sizeof(TUpdSlot) == 64 &&
	sizeof(TUpdEnt) == 16, "record sizes");

// one pass over the stages: with hand-ups or without
class CPanelPass {
	const Plan &P;
	const SparseRecordOptions &t_opt;
	SparseRecords &R;
	SparseLaunchLists &L;
	const int n_stages, n_slot_cap;
	const int64_t n_lblocks;
	const bool b_hand_up; // this pass hands up at all
	const int n_handup_max_tasks, n_ride_max_fresh;
	std::vector<int32_t> col_local, col_stage;
	std::vector<int32_t> slot_of; // factor block -> slot of the task being packed (else -1)
	// round 4, hand-ups (TPanelOut): the slot every factor block has in the image of its own task, once that task's package
	// exists (-1: the task went to the column kernel), the package of every column's task, and per package what it hands up
	std::vector<int32_t> img_slot, col_package, col_level; // (col_level: which of its task's levels a column is in)
	struct THandUp { std::vector<TPanelOut> recs; std::vector<uint32_t> pairs; };
	std::vector<THandUp> hand_up; // indexed by package
	std::map<std::pair<int32_t, int64_t>, int32_t> out_of; // (source package, target factor block) -> record of that package
	// the stage being packed: what Decide_Stage() found
	int s;
	bool b_panel_stage, b_hand_up_stage;
	int n_stage_waves;
	int64_t n_stage_max_slots, n_stage_max_units, n_stage_rest; // (for the development print)
	int n_stage_bwd_units, n_stage_bwd_blocks, n_stage_bwd_levels; // (the same for the backward records: largest record, most blocks below a diagonal, most levels)
	enum { FETCH_MAX_PASS = 8 };
	int64_t n_stage_fetch_mod[FETCH_MAX_PASS], n_stage_fetch_few[FETCH_MAX_PASS]; // (the same for the fresh entries a wave fetches itself, kinds 0 / 1: waves by their count modulo the packed fetch's pass -- panel_fetch_pass() of the stage's waves --, waves with fewer than a pass by their count)
	int n_stage_fetch_min, n_stage_fetch_max;
	// the task being packed: what Size_Task() found
	std::vector<int64_t> order; // the task's columns (indices into cols) level by level
	bool b_tall;
	int64_t n_slots, n_fresh;
	size_t n_units;
	std::vector<TPanelExt> fresh;
	std::vector<uint32_t> irow, ipair;
	std::vector<TPanelCol> pcols;
	std::vector<TPanelSlot> pslots;

public:
	CPanelPass(const Plan &r_plan, const SparseRecordOptions &r_opt, SparseRecords &r_rec, SparseLaunchLists &r_lists, bool b_hand_up_allowed)
		:P(r_plan), t_opt(r_opt), R(r_rec), L(r_lists), n_stages(int(P.stage_ptr.size()) - 1), n_slot_cap(panel_slot_cap(P.max_dim)),
		n_lblocks(int64_t(P.lrow.size())), b_hand_up(b_hand_up_allowed),
		n_handup_max_tasks(dev_knob("SLAMPP_HIP_DEV_HANDUP_MAX_TASKS", 1 << 30)), // (measured at C3: handing up from the 2 420-task stage as well 224 -> 208 us for the separator launches, from the narrow stages only 224 -> 214)
		n_ride_max_fresh(dev_knob("SLAMPP_HIP_DEV_PANEL_RIDE_FRESH", 96)),
		col_local(size_t(P.n), -1), col_stage(size_t(P.n), -1), slot_of(size_t(n_lblocks), -1),
		img_slot(size_t(n_lblocks), -1), col_package(size_t(P.n), -1), col_level(size_t(P.n), 0)
	{}

	void Run()
	{
		// the leaf subtrees too, where they are so few that one round of workgroups takes them all: a small system's leaf
		// stage is all latency, and eight waves on a subtree of four columns beat one (37 -> 19 us on the reduced camera
		// system of C4; with 1 600 leaf tasks -- 10 000 poses -- the wave-per-task kernel wins again, 0.33 against 0.38 ms)
		const bool b_leaf_panels = n_stages > 0 && t_opt.n_simt <= 0 && P.stage_ptr[1] - P.stage_ptr[0] <= 512; // (one round of workgroups)
		L.panel_ptr.assign(n_stages + 1, 0);
		L.panel_rest_ptr.assign(n_stages + 1, 0);
		L.panel_upd_ptr.assign(n_stages + 1, 0);
		for(int n_stage = 0; n_stage < n_stages; ++ n_stage) {
			for(int64_t i = P.task_ptr[P.stage_ptr[n_stage]]; i < P.task_ptr[P.stage_ptr[n_stage + 1]]; ++ i)
				col_stage[P.task_cols[i]] = n_stage;
		}
		L.panel_ride.assign(n_stages + 1, 0);
		L.panel_cfg.assign(size_t(n_stages) + 1, TPanelLaunch{int32_t(PANEL_W), int32_t(64 * PANEL_W), 1, 1, 1, 0});
		L.bwd_cfg.assign(size_t(n_stages) + 1, TBwdLaunch{1, 1, 4});
		for(s = 0; s < n_stages; ++ s) {
			b_panel_stage = s >= L.n_bottom_stages || (s == 0 && b_leaf_panels);
			Decide_Stage();
			n_stage_max_slots = n_stage_max_units = n_stage_rest = 0;
			n_stage_bwd_units = n_stage_bwd_blocks = n_stage_bwd_levels = 0;
			for(int i = 0; i < FETCH_MAX_PASS; ++ i)
				n_stage_fetch_mod[i] = n_stage_fetch_few[i] = 0;
			n_stage_fetch_min = INT_MAX;
			n_stage_fetch_max = 0;
			for(int t = P.stage_ptr[s]; b_panel_stage && t < P.stage_ptr[s + 1]; ++ t) {
				if(Size_Task(t))
					Pack_Task(t);
				else
					R.panel_rest.push_back(t);
			}
			L.panel_ptr[s + 1] = int32_t(R.panel_off.size());
			Write_Hand_Up_Lists();
			if(t_opt.b_timing && b_panel_stage)
				fprintf(stderr, "[setup] stage %d panels: at most %lld blocks and %lld package units per task, %lld tasks left to the column kernel\n",
					s, (long long)n_stage_max_slots, (long long)n_stage_max_units, (long long)n_stage_rest);
			if(t_opt.b_timing && L.panel_ptr[s + 1] > L.panel_ptr[s]) {
				const int n_pass = std::min(panel_fetch_pass(n_stage_waves), int(FETCH_MAX_PASS));
				fprintf(stderr, "[setup] stage %d fresh fetch: %d waves a task, pass of %d, %d to %d self-fetched entries per wave; waves by entries modulo the pass:",
					s, n_stage_waves, n_pass, n_stage_fetch_min, n_stage_fetch_max);
				for(int i = 0; i < n_pass; ++ i)
					fprintf(stderr, " %lld", (long long)n_stage_fetch_mod[i]);
				fprintf(stderr, "; waves with fewer than a pass, by entries:");
				for(int i = 0; i < n_pass; ++ i)
					fprintf(stderr, " %lld", (long long)n_stage_fetch_few[i]);
				fprintf(stderr, "\n");
			}
			if(t_opt.b_timing && L.panel_ptr[s + 1] > L.panel_ptr[s])
				fprintf(stderr, "[setup] stage %d backward records: %d tasks, at most %d units, %d blocks below a diagonal and %d levels per task; %d columns per wave\n",
					s, int(L.panel_ptr[s + 1] - L.panel_ptr[s]), n_stage_bwd_units, n_stage_bwd_blocks, n_stage_bwd_levels, int(L.bwd_cfg[s].n_cols_per_wave));
			L.panel_rest_ptr[s + 1] = int32_t(R.panel_rest.size());
			L.panel_upd_ptr[s + 1] = int32_t(R.upd_slots.size());
		}
		if(R.panel_off.empty()) {
			L.panel_ptr.clear();
			L.panel_rest_ptr.clear();
			L.panel_upd_ptr.clear();
		} else
			R.panel_pkg.resize(R.panel_pkg.size() + 64 * PANEL_W, longlong2{0, 0}); // speculative reads past the last package
	}

private:
	// an update whose operands a task of the stage right below keeps in its image is handed up by that task (one
	// ready-made block per source task and target block) instead of fetched and multiplied here
	bool b_Handed_Up(int64_t n_operand_blk) const
	{
		return b_hand_up_stage && L.panel_ride[s] != 2 && img_slot[n_operand_blk] >= 0 && col_stage[P.blk_col[n_operand_blk]] == s - 1;
	}

	// the stage's launch: waves per task, and whether its updates from further down ride in the launch of the stage below,
	// get a launch of their own, or are brought in by the tasks themselves
	void Decide_Stage()
	{
		// Do this stage's updates from further down ride in the launch of the stage below?  Only if that is a panel launch,
		// and only if what is then left to the tasks themselves -- the updates from the stage right below -- is little:
		// a task brings those in with its own eight waves, on the stage's critical path (a launch saved is about 4 us)
		// Waves per task: eight where the stage is a launch on the critical path, four where it holds more tasks than the
		// chip takes at once (more workgroups per CU: throughput), two where it holds them several times over.
		// (round 4: two where it holds them several times over -- C3's 2 151-task launch 91 -> 78 us, the step 0.330 -> 0.318 ms;
		// a million poses 2.185 -> 2.146; one wave per task is slower again, 169 against 147 us for C3's slice launches, and two
		// waves for the 303-task launch as well 153: the development knobs below moved the lines)
		const int n_w4_min_tasks = dev_knob("SLAMPP_HIP_DEV_PANEL_W4_MIN", 512);
		const int n_w2_min_tasks = dev_knob("SLAMPP_HIP_DEV_PANEL_W2_MIN", 1024);
		n_stage_waves = (b_panel_stage && P.stage_ptr[s + 1] - P.stage_ptr[s] > n_w2_min_tasks)? 2 :
			(b_panel_stage && P.stage_ptr[s + 1] - P.stage_ptr[s] > n_w4_min_tasks)? 4 : int(PANEL_W);
		// hand-ups from the stage below (development knob SLAMPP_HIP_DEV_HANDUP_MAX_TASKS: only from stages of at most that many tasks --
		// a stage that fills the chip several times over is bound by throughput, and what its tasks compute for the stage
		// above they compute instead of the next task's columns: C3's 2 420-task launch 70 -> 92 us; the stage above gains more)
		b_hand_up_stage = b_hand_up && s > 0 && P.stage_ptr[s] - P.stage_ptr[s - 1] <= n_handup_max_tasks;
		L.panel_cfg[s].n_waves = n_stage_waves;
		// the backward launch of the stage (backward_slice_kernel): a wave owns one column of its task where the stage is a
		// launch on the critical path, two or four where it is crowded; the waves per task follow from the stage's tasks
		// (measured at C3's 2 066-task stage: four, two and one column per wave all take 14 - 15 us where the column kernel takes
		// 11.6 -- the shape does not decide there; option panel_backward = -1 leaves such a stage to the column kernel)
		L.bwd_cfg[s] = TBwdLaunch{1, int32_t(PANEL_W) / n_stage_waves, 4};
		L.panel_cfg[s].n_cap_units = 64 * n_stage_waves; // (one speculative unit per thread)
		// The first stage above a leaf stage that is not a panel launch: everything its tasks receive comes from that one
		// stage, nothing from further down -- the tasks bring it in themselves and no update launch is needed (if it fits
		// the packages: the tall tasks of a wide stage receive some fifty products each)
		// ... Or do the tasks bring in everything themselves (mode 2: they read Lambda and all their updates, no update role
		// has prepared their blocks)?  Where the launch below is no panel launch (the first stage above lane-per-task
		// leaves: everything comes from that one stage), and where it is so crowded -- more workgroups than the chip holds at
		// once -- that riders only make it longer (C3: 5 816 riders in the 2 420-task stage cost it 20 us; the 625 tasks
		// above them take their ~150 products each in 6) -- if it fits the packages.
		const std::vector<int32_t> &panel_ptr = L.panel_ptr;
		const bool b_first_above_leaves = b_panel_stage && s == 1 && panel_ptr[1] == panel_ptr[0];
		// (measured at C3 and not kept as the default: without its 5 816 riders the 2 420-task launch takes the same 67 us --
		// its own tasks fill the chip for that long --, and the stage above, bringing in ~150 products a task, 32 instead of 23)
		const bool b_below_crowded = dev_knob_set("SLAMPP_HIP_DEV_PANEL_SELF_ABOVE_CROWDED") && b_panel_stage && s > 0 && panel_ptr[s] - panel_ptr[s - 1] > 1024;
		if(!(b_panel_stage && s > 0 && (panel_ptr[s] > panel_ptr[s - 1] || b_first_above_leaves)))
			return;
		int64_t n_max_fresh = 0, n_max_external = 0;
		for(int t = P.stage_ptr[s]; t < P.stage_ptr[s + 1]; ++ t) {
			int64_t n_task_fresh = 0, n_external = 0;
			for(int64_t i = P.task_ptr[t]; i < P.task_ptr[t + 1]; ++ i) {
				const TColDesc &c = R.cols[i];
				for(int64_t e = c.r0; e < c.r0 + c.nr; ++ e) {
					const bool b_up = b_hand_up_stage && img_slot[P.rblk[e]] >= 0 && col_stage[P.blk_col[P.rblk[e]]] == s - 1;
					n_task_fresh += !b_up && col_stage[P.blk_col[P.rblk[e]]] == s - 1;
					n_external += !b_up && col_stage[P.blk_col[P.rblk[e]]] < s;
				}
				for(int64_t e = P.pptr[c.k0 + 1]; e < P.pptr[c.k0 + c.nb]; ++ e) {
					const bool b_up = b_hand_up_stage && img_slot[P.pa[e]] >= 0 && col_stage[P.blk_col[P.pa[e]]] == s - 1;
					n_task_fresh += !b_up && col_stage[P.blk_col[P.pa[e]]] == s - 1;
					n_external += !b_up && col_stage[P.blk_col[P.pa[e]]] < s;
				}
			}
			n_max_fresh = std::max(n_max_fresh, n_task_fresh);
			n_max_external = std::max(n_max_external, n_external);
		}
		if((b_first_above_leaves || b_below_crowded) && n_max_external <= 320)
			L.panel_ride[s] = 2;
		else if(panel_ptr[s] > panel_ptr[s - 1])
			L.panel_ride[s] = n_max_fresh <= n_ride_max_fresh;
		L.panel_cfg[s].b_from_lambda = L.panel_ride[s] == 2;
		if(t_opt.b_timing)
			fprintf(stderr, "[setup] stage %d: %d tasks, at most %lld updates from the stage below, %lld in all: %s\n", s,
				P.stage_ptr[s + 1] - P.stage_ptr[s], (long long)n_max_fresh, (long long)n_max_external,
				(L.panel_ride[s] == 2)? "the tasks bring them in" : L.panel_ride[s]? "ride" : "own launch");
	}

	void Release_Slots()
	{
		for(size_t o = 0; o < order.size(); ++ o) {
			const TColDesc &c = R.cols[order[o]];
			for(int64_t k = c.k0; k < c.k0 + c.nb; ++ k)
				slot_of[k] = -1;
		}
	}

	// the order of the task's columns, the slots of its blocks (slot_of) and the size of its package; false: the task does
	// not fit the panel kernel (slot_of is clean again)
	bool Size_Task(int t)
	{
		const int64_t c_begin = P.task_ptr[t], c_end = P.task_ptr[t + 1];
		const int n_cols = int(c_end - c_begin);
		bool b_fits = n_cols >= 1 && n_cols <= int(PANEL_COLS);
		// the package lists the task's columns level by level (a tall task: Plan::col_sub; a chain: one column per
		// level, in order), the slots of the LDS image are their blocks in that order
		order.clear();
		for(int64_t i = c_begin; i < c_end; ++ i)
			order.push_back(i);
		b_tall = false;
		for(int64_t i = c_begin; i < c_end; ++ i)
			b_tall = b_tall || P.col_sub[P.task_cols[i]] != 0;
		if(b_tall) {
			std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
				return P.col_sub[P.task_cols[a]] < P.col_sub[P.task_cols[b]]; });
		}
		n_slots = 0;
		int64_t n_int_rows = 0, n_int_pairs = 0;
		for(size_t o = 0; b_fits && o < order.size(); ++ o)
			n_slots += R.cols[order[o]].nb;
		b_fits = b_fits && n_slots <= n_slot_cap;
		if(b_fits) {
			int32_t n_slot = 0;
			for(size_t o = 0; o < order.size(); ++ o) {
				const TColDesc &c = R.cols[order[o]];
				for(int64_t k = c.k0; k < c.k0 + c.nb; ++ k)
					slot_of[k] = n_slot ++;
			}
		}
		// the updates from stages further down are applied inside the launch of the stage below, if that is a panel
		// launch: then what the stage right below contributes ("fresh") is left to the task itself
		const bool b_ride = L.panel_ride[s] != 0, b_self = L.panel_ride[s] == 2;
		n_fresh = 0;
		std::vector<std::pair<int32_t, int64_t> > up_keys; // (source package, target block) of this task's hand-ups, in order of first use
		auto Count_Up = [&](int64_t n_operand_blk, int64_t n_target_blk) {
			const std::pair<int32_t, int64_t> key(col_package[P.blk_col[n_operand_blk]], n_target_blk);
			if(std::find(up_keys.begin(), up_keys.end(), key) == up_keys.end())
				up_keys.push_back(key);
		};
		for(int64_t i = c_begin; b_fits && i < c_end; ++ i) { // size of the package
			const TColDesc &c = R.cols[i];
			for(int64_t e = c.r0; e < c.r0 + c.nr; ++ e) {
				const bool b_int = slot_of[P.rblk[e]] >= 0;
				n_int_rows += b_int;
				if(!b_int && b_Handed_Up(P.rblk[e]))
					Count_Up(P.rblk[e], c.k0);
				else
					n_fresh += !b_int && b_ride && (b_self || col_stage[P.blk_col[P.rblk[e]]] == s - 1);
			}
			for(int64_t k = c.k0 + 1; k < c.k0 + c.nb; ++ k) {
				for(int64_t e = P.pptr[k]; e < P.pptr[k + 1]; ++ e) {
					const bool b_int = slot_of[P.pa[e]] >= 0;
					n_int_pairs += b_int;
					if(!b_int && b_Handed_Up(P.pa[e]))
						Count_Up(P.pa[e], k);
					else
						n_fresh += !b_int && b_ride && (b_self || col_stage[P.blk_col[P.pa[e]]] == s - 1);
				}
			}
		}
		n_fresh += int64_t(up_keys.size());
		n_units = 4 + 3 * size_t(n_cols) + 2 * size_t(n_slots) + size_t(n_int_rows + 3) / 4 + size_t(n_int_pairs + 3) / 4 +
			2 * size_t(n_fresh);
		b_fits = b_fits && n_units <= size_t(PANEL_UNITS);
		n_stage_max_slots = std::max(n_stage_max_slots, n_slots);
		n_stage_max_units = std::max(n_stage_max_units, int64_t(n_units));
		n_stage_rest += !b_fits;
		if(!b_fits && n_slots <= n_slot_cap && n_cols >= 1 && n_cols <= int(PANEL_COLS))
			Release_Slots();
		return b_fits;
	}

	// one more operand pair for the block the source task hands up for target block n_target (a new record there, and
	// the entry here that subtracts it, when it is the first)
	void Hand_Up(int64_t ka, int64_t kb, int64_t n_target, int32_t n_col_here, int32_t n_slot_here, bool b_diag)
	{
		const int32_t n_src = col_package[P.blk_col[ka]];
		const std::pair<int32_t, int64_t> key(n_src, n_target);
		std::map<std::pair<int32_t, int64_t>, int32_t>::iterator it = out_of.find(key);
		THandUp &r_up = hand_up[size_t(n_src)];
		if(it == out_of.end()) {
			TPanelOut rec;
			rec.op0 = -1; // (the pairs of a record are collected apart and laid out when the list is written)
			rec.onp = 0;
			rec.dst = R.n_handup_doubles | (int64_t(b_diag) << 62);
			it = out_of.insert(std::make_pair(key, int32_t(r_up.recs.size()))).first;
			r_up.recs.push_back(rec);
			TPanelExt en;
			memset(&en, 0, sizeof(en));
			en.a_off = R.n_handup_doubles;
			en.slot = uint16_t(n_slot_here);
			en.kind = b_diag? 3 : 2;
			en.col = n_col_here;
			fresh.push_back(en);
			R.n_handup_doubles += P.max_dim * P.max_dim + 8;
		}
		// (until the list is written, onp holds the last of the source task's levels the record's operands come from)
		r_up.recs[size_t(it->second)].onp = std::max(r_up.recs[size_t(it->second)].onp, col_level[P.blk_col[ka]]);
		r_up.pairs.push_back(uint32_t(it->second));
		r_up.pairs.push_back(b_diag? (uint32_t(img_slot[ka]) | (uint32_t(col_local[P.blk_col[ka]]) << 16)) :
			(uint32_t(img_slot[ka]) | (uint32_t(img_slot[kb]) << 16)));
	}

	// the package of a task Size_Task() has accepted, the update lists of its blocks, and what it asks of the tasks below
	void Pack_Task(int t)
	{
		const int n_cols = int(P.task_ptr[t + 1] - P.task_ptr[t]);
		const bool b_ride = L.panel_ride[s] != 0, b_self = L.panel_ride[s] == 2;
		irow.clear(); ipair.clear(); pcols.clear(); pslots.clear(); fresh.clear();
		for(size_t o = 0; o < order.size(); ++ o)
			col_local[P.task_cols[order[o]]] = int32_t(o);
		for(size_t o = 0; o < order.size(); ++ o) {
			const int64_t i = order[o];
			const TColDesc &c = R.cols[i];
			TPanelCol pc;
			memset(&pc, 0, sizeof(pc));
			pc.linv_off = c.linv_off;
			pc.cs_new = c.cs_new;
			pc.cs_src = c.cs_src;
			pc.slot0 = slot_of[c.k0];
			pc.nb = c.nb;
			pc.sub = b_tall? P.col_sub[P.task_cols[i]] : int32_t(o); // (a chain: every column a level of its own)
			pc.ir0 = int32_t(irow.size());
			TUpdSlot us;
			memset(&us, 0, sizeof(us));
			us.loff = R.blks[c.k0].loff;
			us.asrc = R.blks[c.k0].asrc;
			us.e0 = int64_t(R.upd_ents.size());
			us.kind = 1;
			us.cs_src = c.cs_src;
			us.cs_new = c.cs_new;
			for(int64_t e = c.r0; e < c.r0 + c.nr; ++ e) { // row entries of the diagonal block: blocks L(j,c)
				const int64_t k = P.rblk[e];
				if(slot_of[k] >= 0)
					irow.push_back(uint32_t(slot_of[k]) | (uint32_t(col_local[P.blk_col[k]]) << 16));
				else if(b_Handed_Up(k))
					Hand_Up(k, k, c.k0, int32_t(o), pc.slot0, true);
				else if(b_ride && (b_self || col_stage[P.blk_col[k]] == s - 1)) {
					TPanelExt en;
					memset(&en, 0, sizeof(en));
					en.a_off = en.b_off = R.rents[e].off;
					en.ycs = R.rents[e].ycs;
					en.slot = uint16_t(pc.slot0);
					en.kind = 1;
					en.col = int32_t(o);
					fresh.push_back(en);
				} else
					R.upd_ents.push_back(TUpdEnt{R.rents[e].off, int64_t(R.rents[e].ycs)});
			}
			us.ne = int32_t(int64_t(R.upd_ents.size()) - us.e0);
			R.upd_slots.push_back(us);
			pc.inr = int32_t(irow.size()) - pc.ir0;
			pcols.push_back(pc);
			for(int64_t k = c.k0; k < c.k0 + c.nb; ++ k) {
				TPanelSlot ps;
				memset(&ps, 0, sizeof(ps));
				ps.loff = R.blks[k].loff;
				ps.asrc = R.blks[k].asrc;
				ps.ip0 = int32_t(ipair.size());
				if(k > c.k0) { // (the diagonal block's updates are its row entries)
					memset(&us, 0, sizeof(us));
					us.loff = R.blks[k].loff;
					us.asrc = R.blks[k].asrc;
					us.e0 = int64_t(R.upd_ents.size());
					for(int64_t e = P.pptr[k]; e < P.pptr[k + 1]; ++ e) {
						const int64_t ka = P.pa[e], kb = P.pb[e];
						if(slot_of[ka] >= 0)
							ipair.push_back(uint32_t(slot_of[ka]) | (uint32_t(slot_of[kb]) << 16));
						else if(b_Handed_Up(ka))
							Hand_Up(ka, kb, k, 0, slot_of[k], false);
						else if(b_ride && (b_self || col_stage[P.blk_col[ka]] == s - 1)) {
							TPanelExt en;
							memset(&en, 0, sizeof(en));
							en.a_off = P.loff[ka];
							en.b_off = P.loff[kb];
							en.slot = uint16_t(slot_of[k]);
							fresh.push_back(en);
						} else
							R.upd_ents.push_back(TUpdEnt{P.loff[ka], P.loff[kb]});
					}
					us.ne = int32_t(int64_t(R.upd_ents.size()) - us.e0);
					R.upd_slots.push_back(us);
				}
				ps.inp = int32_t(ipair.size()) - ps.ip0;
				pslots.push_back(ps);
			}
		}
		if(int64_t(fresh.size()) != n_fresh)
			throw std::logic_error("panel package: fresh entries miscounted");
		Append_Package(n_cols);
		Append_Backward_Record();
		for(size_t o = 0, n_level = 0; o < order.size(); ++ o) {
			const TColDesc &c = R.cols[order[o]];
			for(int64_t k = c.k0; k < c.k0 + c.nb; ++ k)
				img_slot[k] = slot_of[k];
			col_package[P.task_cols[order[o]]] = int32_t(R.panel_off.size()) - 1;
			if(o > 0 && pcols[o].sub != pcols[o - 1].sub)
				++ n_level;
			col_level[P.task_cols[order[o]]] = int32_t(n_level);
		}
		Release_Slots();
	}

	// lays the task's records into panel_pkg: head | columns | slots | internal row entries | internal pairs | fresh entries
	void Append_Package(int n_cols)
	{
		TPanelHead hd;
		memset(&hd, 0, sizeof(hd));
		hd.n_cols = n_cols;
		hd.n_slots = int32_t(n_slots);
		hd.n_units = int32_t(n_units);
		hd.n_int_rows = int32_t(irow.size());
		// fresh entries by the wave that owns their slot, inside a wave by slot, inside a slot in list order
		// (of a wave's entries the handed-up blocks first: the kernel takes them eight at a time)
		const int n_waves = n_stage_waves;
		std::stable_sort(fresh.begin(), fresh.end(), [n_waves](const TPanelExt &x, const TPanelExt &y) {
			const int wx = x.slot % n_waves, wy = y.slot % n_waves, ux = x.kind < 2, uy = y.kind < 2;
			return wx < wy || (wx == wy && (ux < uy || (ux == uy && x.slot < y.slot))); });
		for(size_t e = 0; e < fresh.size(); ++ e)
			++ hd.ext_ptr[fresh[e].slot % n_waves + 1];
		for(int v = 0; v < n_waves; ++ v)
			hd.ext_ptr[v + 1] += hd.ext_ptr[v];
		for(int v = 0; t_opt.b_timing && v < n_waves; ++ v) { // (development print: what the fetch loop of each wave gets)
			int n_self = 0;
			for(int e = hd.ext_ptr[v]; e < hd.ext_ptr[v + 1]; ++ e)
				n_self += fresh[size_t(e)].kind < 2;
			const int n_pass = std::min(panel_fetch_pass(n_waves), int(FETCH_MAX_PASS));
			++ n_stage_fetch_mod[n_self % n_pass];
			if(n_self < n_pass)
				++ n_stage_fetch_few[n_self];
			n_stage_fetch_min = std::min(n_stage_fetch_min, n_self);
			n_stage_fetch_max = std::max(n_stage_fetch_max, n_self);
		}
		{ // what the stage's launch must hold
			TPanelLaunch &r_cfg = L.panel_cfg[s];
			r_cfg.n_cap_units = std::max(r_cfg.n_cap_units, int32_t(n_units));
			r_cfg.n_cap_blk = std::max(r_cfg.n_cap_blk, int32_t(n_slots));
			r_cfg.n_cap_cols = std::max(r_cfg.n_cap_cols, int32_t(n_cols));
			int n_level_cols = 0, n_level = -1;
			for(size_t o = 0; o < pcols.size(); ++ o) {
				n_level_cols = (pcols[o].sub == n_level)? n_level_cols + 1 : 1;
				n_level = pcols[o].sub;
				r_cfg.n_cap_lvl = std::max(r_cfg.n_cap_lvl, int32_t(n_level_cols));
			}
		}
		const size_t n_at = R.panel_pkg.size();
		R.panel_pkg.resize(n_at + n_units, longlong2{0, 0});
		char *p_dst = reinterpret_cast<char*>(&R.panel_pkg[n_at]);
		memcpy(p_dst, &hd, sizeof(hd));
		p_dst += 64;
		memcpy(p_dst, pcols.data(), pcols.size() * sizeof(TPanelCol));
		p_dst += pcols.size() * sizeof(TPanelCol);
		memcpy(p_dst, pslots.data(), pslots.size() * sizeof(TPanelSlot));
		p_dst += pslots.size() * sizeof(TPanelSlot);
		if(!irow.empty())
			memcpy(p_dst, irow.data(), irow.size() * sizeof(uint32_t));
		p_dst += (irow.size() + 3) / 4 * 16;
		if(!ipair.empty())
			memcpy(p_dst, ipair.data(), ipair.size() * sizeof(uint32_t));
		p_dst += (ipair.size() + 3) / 4 * 16;
		if(!fresh.empty())
			memcpy(p_dst, fresh.data(), fresh.size() * sizeof(TPanelExt));
		R.panel_off.push_back(int64_t(n_at));
		R.panel_out_off.push_back(-1);
		R.panel_units.push_back(int32_t(n_units));
		hand_up.push_back(THandUp());
	}

	// the task's backward record (TBwdHead: sparse_kernels.h): its columns level by level as in the package, and per
	// sub-diagonal block where the x of its row comes from -- a column of a later level of this task, or the workspace
	void Append_Backward_Record()
	{
		TBwdHead hd;
		memset(&hd, 0, sizeof(hd));
		std::vector<TBwdCol> bcols;
		std::vector<TBwdBlk> bblks;
		for(size_t o = 0; o < order.size(); ++ o) {
			const TColDesc &c = R.cols[order[o]];
			if(o > 0 && pcols[o].sub != pcols[o - 1].sub)
				++ hd.n_levels;
			hd.lvl_ptr[hd.n_levels + 1] = int32_t(o) + 1;
			TBwdCol bc;
			bc.linv_off = c.linv_off;
			bc.cs_src = c.cs_src;
			bc.cs_new = int32_t(c.cs_new);
			bc.blk0 = int32_t(bblks.size());
			bc.nb = c.nb - 1;
			bc.level = hd.n_levels;
			bcols.push_back(bc);
			for(int64_t k = c.k0 + 1; k < c.k0 + c.nb; ++ k) {
				const int32_t n_row = P.lrow[k];
				TBwdBlk bb;
				bb.loff = R.blks[k].loff;
				bb.xsrc = R.blks[k].xcs;
				bb.pad = 0;
				if(slot_of[P.lptr[n_row]] >= 0) { // (the row is a column of this task: col_local is this task's, set by Pack_Task)
					const int32_t n_local = col_local[n_row];
					if(n_local <= int32_t(o) || pcols[size_t(n_local)].sub == pcols[o].sub)
						throw std::logic_error("backward record: a block's row is not in a later level of its task");
					bb.xsrc = ~n_local;
				}
				bblks.push_back(bb);
			}
		}
		++ hd.n_levels;
		hd.n_cols = int32_t(order.size());
		hd.n_blks = int32_t(bblks.size());
		hd.n_units = int32_t(4 + 2 * bcols.size() + bblks.size());
		n_stage_bwd_units = std::max(n_stage_bwd_units, int(hd.n_units));
		n_stage_bwd_levels = std::max(n_stage_bwd_levels, int(hd.n_levels));
		for(size_t o = 0; o < bcols.size(); ++ o)
			n_stage_bwd_blocks = std::max(n_stage_bwd_blocks, int(bcols[o].nb));
		TBwdLaunch &r_cfg = L.bwd_cfg[s];
		r_cfg.n_cap_units = std::max(r_cfg.n_cap_units, hd.n_units);
		r_cfg.n_waves = std::max(r_cfg.n_waves, (hd.n_cols + r_cfg.n_cols_per_wave - 1) / r_cfg.n_cols_per_wave);
		const size_t n_at = R.bwd_rec.size();
		R.bwd_rec.resize(n_at + size_t(hd.n_units), longlong2{0, 0});
		char *p_dst = reinterpret_cast<char*>(&R.bwd_rec[n_at]);
		memcpy(p_dst, &hd, sizeof(hd));
		memcpy(p_dst + 64, bcols.data(), bcols.size() * sizeof(TBwdCol));
		if(!bblks.empty())
			memcpy(p_dst + 64 + bcols.size() * sizeof(TBwdCol), bblks.data(), bblks.size() * sizeof(TBwdBlk));
		R.bwd_off.push_back(int64_t(n_at) | (int64_t(hd.n_units) << BWD_OFF_BITS));
	}

	// the hand-up lists of the stage below (its packages exist already: the lists go behind this stage's, the heads are told)
	void Write_Hand_Up_Lists()
	{
		for(int32_t n_pkg = (s > 0)? L.panel_ptr[s - 1] : 0; s > 0 && n_pkg < L.panel_ptr[s]; ++ n_pkg) {
			THandUp &r_up = hand_up[size_t(n_pkg)];
			if(r_up.recs.empty())
				continue;
			// the list: [12 x int32: records whose operands are final after level 0, 1, ...][records, in that order][their pairs] --
			// the waves a level's column work leaves idle take the records that are ready, the rest is done at the end
			const size_t n_out = r_up.recs.size(), n_pairs = r_up.pairs.size() / 2;
			enum { OUT_LEVELS = 12 };
			std::vector<int32_t> rec_order(n_out), rec_new(n_out), level_end(OUT_LEVELS, 0);
			for(size_t o = 0; o < n_out; ++ o)
				rec_order[o] = int32_t(o);
			std::stable_sort(rec_order.begin(), rec_order.end(), [&](int32_t a, int32_t b) { return r_up.recs[size_t(a)].onp < r_up.recs[size_t(b)].onp; });
			for(size_t o = 0; o < n_out; ++ o) {
				rec_new[size_t(rec_order[o])] = int32_t(o);
				for(int l = std::min(r_up.recs[size_t(rec_order[o])].onp, int32_t(OUT_LEVELS) - 1); l < int(OUT_LEVELS); ++ l)
					++ level_end[size_t(l)];
			}
			std::vector<TPanelOut> recs_sorted(n_out);
			for(size_t o = 0; o < n_out; ++ o)
				recs_sorted[o] = r_up.recs[size_t(rec_order[o])];
			std::vector<uint32_t> sorted(n_pairs);
			{
				std::vector<int32_t> count(n_out + 1, 0);
				for(size_t e = 0; e < n_pairs; ++ e)
					++ count[size_t(rec_new[r_up.pairs[2 * e]]) + 1];
				for(size_t o = 0; o < n_out; ++ o) {
					recs_sorted[o].op0 = count[o];
					recs_sorted[o].onp = count[o + 1];
					count[o + 1] += count[o];
				}
				std::vector<int32_t> fill(count.begin(), count.end() - 1);
				for(size_t e = 0; e < n_pairs; ++ e) // (stable: the pairs of a record keep their order)
					sorted[size_t(fill[size_t(rec_new[r_up.pairs[2 * e]])] ++)] = r_up.pairs[2 * e + 1];
			}
			const size_t n_list_units = 3 + n_out + (n_pairs + 3) / 4;
			const size_t n_at = R.panel_pkg.size();
			R.panel_pkg.resize(n_at + n_list_units, longlong2{0, 0});
			memcpy(&R.panel_pkg[n_at], level_end.data(), OUT_LEVELS * sizeof(int32_t));
			memcpy(&R.panel_pkg[n_at + 3], recs_sorted.data(), n_out * sizeof(TPanelOut));
			if(n_pairs)
				memcpy(&R.panel_pkg[n_at + 3 + n_out], sorted.data(), n_pairs * sizeof(uint32_t));
			R.panel_out_off[size_t(n_pkg)] = int64_t(n_at);
			TPanelHead *p_head = reinterpret_cast<TPanelHead*>(&R.panel_pkg[size_t(R.panel_off[size_t(n_pkg)])]);
			p_head->ext_ptr[10] = int32_t(n_out);
			p_head->ext_ptr[11] = int32_t(n_list_units);
			L.panel_cfg[s - 1].n_cap_out = std::max(L.panel_cfg[s - 1].n_cap_out, int32_t(n_list_units));
			L.b_any_hand_up = true;
			{ THandUp t_empty; std::swap(r_up, t_empty); }
		}
		out_of.clear();
	}
};

// all packages and lists of one pass; returns whether every stage's launch fits the LDS budget
bool b_Panel_Pass(const Plan &P, const SparseRecordOptions &t_opt, SparseRecords &R, SparseLaunchLists &L, bool b_hand_up_allowed)
{
	R.panel_pkg.clear();
	R.panel_off.clear();
	R.panel_out_off.clear();
	R.panel_units.clear();
	R.bwd_rec.clear();
	R.bwd_off.clear();
	L.bwd_cfg.clear();
	R.n_handup_doubles = 0;
	R.panel_rest.clear();
	R.upd_slots.clear();
	R.upd_ents.clear();
	L.panel_ptr.clear();
	L.panel_rest_ptr.clear();
	L.panel_upd_ptr.clear();
	L.b_any_hand_up = false;
	if(t_opt.n_panel && b_Package_Dim(P))
		CPanelPass(P, t_opt, R, L, b_hand_up_allowed).Run();
	bool b_lds_fits = true;
	for(size_t i = 0; i < L.panel_cfg.size() && !R.panel_off.empty(); ++ i) {
		b_lds_fits = b_lds_fits && size_t(panel_lds(P.max_dim, true, L.panel_cfg[i]).TOTAL) * sizeof(double) <= PANEL_LDS_BUDGET;
		if(t_opt.b_timing && i + 1 < L.panel_ptr.size() && L.panel_ptr[i + 1] > L.panel_ptr[i]) {
			const TPanelLds l = panel_lds(P.max_dim, true, L.panel_cfg[i]);
			fprintf(stderr, "[setup] stage %d panel launch: %d waves a task, LDS %zu bytes (package %d, blocks %d, inverses + tiles %d, operands %d, fresh %d, hand-up list %d doubles)\n",
				int(i), L.panel_cfg[i].n_waves, size_t(l.TOTAL) * sizeof(double), l.IMAGE, l.VEC - l.IMAGE, l.OPS - l.VEC, l.YV - l.OPS, l.OUT - l.YV, l.TOTAL - l.OUT);
		}
	}
	return b_lds_fits;
}

// The launch order inside a stage (round 6): workgroups start in the order of their index, and a launch that holds its
// tasks more than once over (C3's 2 066-task stage: five workgroups a CU by their LDS, two rounds) ends when the last round's
// longest task does.  In the plan's order long and short tasks are mixed, so both rounds last as long as a long task; with the
// big packages first the last round is made of short ones.  Nothing on the host refers to a package by its position
// any more at this point; the device reads pkg_off[blockIdx.x] and out_off[blockIdx.x] only.
void Sort_Launch_Order(SparseRecords &R, const SparseLaunchLists &L)
{
	std::vector<int32_t> order;
	std::vector<int64_t> off_sorted, out_off_sorted, bwd_off_sorted;
	for(size_t st = 0; st + 1 < L.panel_ptr.size(); ++ st) {
		const int32_t n_first = L.panel_ptr[st], n_num = L.panel_ptr[st + 1] - n_first;
		if(n_num < 2)
			continue;
		order.resize(size_t(n_num));
		for(int32_t i = 0; i < n_num; ++ i)
			order[size_t(i)] = n_first + i;
		std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return R.panel_units[size_t(a)] > R.panel_units[size_t(b)]; });
		off_sorted.resize(size_t(n_num));
		out_off_sorted.resize(size_t(n_num));
		bwd_off_sorted.resize(size_t(n_num));
		for(int32_t i = 0; i < n_num; ++ i) {
			off_sorted[size_t(i)] = R.panel_off[size_t(order[size_t(i)])];
			out_off_sorted[size_t(i)] = R.panel_out_off[size_t(order[size_t(i)])];
			bwd_off_sorted[size_t(i)] = R.bwd_off[size_t(order[size_t(i)])];
		}
		std::copy(off_sorted.begin(), off_sorted.end(), R.panel_off.begin() + n_first);
		std::copy(out_off_sorted.begin(), out_off_sorted.end(), R.panel_out_off.begin() + n_first);
		std::copy(bwd_off_sorted.begin(), bwd_off_sorted.end(), R.bwd_off.begin() + n_first);
	}
}

} // anonymous namespace

void build_panel_packages(const Plan &P, const SparseRecordOptions &t_opt, SparseRecords &r_rec, SparseLaunchLists &r_lists)
{
	// (a second pass, without hand-ups, if a stage's hand-up list would take its workgroups past the LDS of a CU: the list
	// rides in the dynamic LDS request on top of the task's image, and nothing else bounds its length -- advisor, round 4)
	const bool b_hand_up = t_opt.n_panel_handup != 0;
	if(!b_Panel_Pass(P, t_opt, r_rec, r_lists, b_hand_up) && b_hand_up)
		b_Panel_Pass(P, t_opt, r_rec, r_lists, false);
	if(dev_knob("SLAMPP_HIP_DEV_PANEL_ORDER", 1) != 0) // (development aid, plan.h: 0 = the plan's order)
		Sort_Launch_Order(r_rec, r_lists);
}

// column packages for the upper stages (see sparse_kernels.h); the limits are those of factor_stage_kernel's staged path
void build_column_packages(const Plan &P, const SparseLaunchLists &r_lists, SparseRecords &r_rec)
{
	raw_vector<longlong2> &pkg = r_rec.pkg;
	std::vector<int64_t> &task_pkg = r_rec.task_pkg;
	pkg.clear();
	task_pkg.assign(P.task_ptr.size() - 1, -1);
	if(!b_Package_Dim(P))
		return;
	const int n_stages = int(P.stage_ptr.size()) - 1;
	// (the wide stages above the leaves and the stages near the root run the same kernel with different capacities)
	const int n_first_stage = (n_stages > 1)? 1 : n_stages;
	for(int t = (n_first_stage < n_stages)? P.stage_ptr[n_first_stage] : int(task_pkg.size()); t < int(task_pkg.size()); ++ t) {
		const bool b_wide = t < P.stage_ptr[std::min(r_lists.n_bottom_stages, n_stages)];
		const int PKG_CHUNK = b_wide? int(WIDE_CHUNK) : int(UP_CHUNK), PKG_NR = b_wide? int(WIDE_NR) : int(UP_NR),
			PKG_NP = b_wide? int(WIDE_NP) : int(UP_NP);
		task_pkg[t] = int64_t(pkg.size());
		for(int64_t i = P.task_ptr[t]; i < P.task_ptr[t + 1]; ++ i) {
			const TColDesc &c = r_rec.cols[i];
			const size_t n_at = pkg.size();
			const bool b_fits = c.nb <= PKG_CHUNK && c.nr <= PKG_NR && c.np <= PKG_NP;
			const int ne = b_fits? c.nr + c.np : 0;
			pkg.resize(n_at + (b_fits? package_units(c.nb, ne) : 4), longlong2{0, 0});
			memcpy(&pkg[n_at], &c, sizeof(TColDesc));
			if(!b_fits)
				continue;
			memcpy(&pkg[n_at + 4], &r_rec.blks[c.k0], size_t(c.nb) * sizeof(TBlkDesc));
			longlong2 *p_ent = &pkg[n_at + 4 + 2 * c.nb];
			int32_t *p_ycs = reinterpret_cast<int32_t*>(p_ent + ne);
			unsigned char *p_tag = reinterpret_cast<unsigned char*>(p_ent + ne + (ne + 3) / 4);
			for(int e = 0; e < c.nr; ++ e) { // row entries of the diagonal block: both operands are the block L(j,c)
				p_ent[e] = longlong2{r_rec.rents[c.r0 + e].off, r_rec.rents[c.r0 + e].off};
				p_ycs[e] = r_rec.rents[c.r0 + e].ycs;
				p_tag[e] = 0;
			}
			for(int e = 0; e < c.np; ++ e) {
				const longlong2 pr = r_rec.pairs[c.p0 + e];
				p_ent[c.nr + e] = longlong2{pr.x & ((int64_t(1) << 48) - 1), pr.y};
				p_tag[c.nr + e] = (unsigned char)((pr.x >> 48) & 0xff);
			}
		}
	}
	pkg.resize(pkg.size() + PKG_SPECULATIVE, longlong2{0, 0});
}

void build_dense_top_records(const Plan &P, int n_dense_pad, SparseRecords &r_rec)
{
	std::vector<TDenseBlk> &dense_blks = r_rec.dense_blks;
	std::vector<TDenseCol> &dense_cols = r_rec.dense_cols;
	dense_blks.clear(); dense_cols.clear(); r_rec.dense_blk_loff.clear();
	r_rec.gaps.clear(); r_rec.unit.clear(); r_rec.dst.clear();
	if(!P.dense_dim)
		return;
	for(int32_t j = 0; j < P.n; ++ j) {
		if(P.dense_pos[j] < 0)
			continue;
		TDenseCol dc;
		dc.cs_new = P.cs_new[j]; dc.cs_src = P.cs_src[j]; dc.pos = P.dense_pos[j]; dc.dj = P.dim[j];
		dense_cols.push_back(dc);
		for(int64_t k = P.lptr[j]; k < P.lptr[j + 1]; ++ k) {
			const int32_t i = P.lrow[k];
			if(P.dense_pos[i] < 0)
				throw std::logic_error("dense top is not closed upwards");
			TDenseBlk b;
			memset(&b, 0, sizeof(b));
			b.asrc = (P.asrc[k] < 0)? -1 : P.asrc[k] * 2 + P.atrans[k];
			b.p0 = P.pptr[k];
			b.np = int32_t(P.pptr[k + 1] - P.pptr[k]);
			b.dst = int64_t(P.dense_pos[i]) + int64_t(P.dense_pos[j]) * n_dense_pad;
			b.di = P.dim[i]; b.dj = P.dim[j];
			if(k == P.lptr[j]) {
				b.r0 = P.rptr[j];
				b.nr = int32_t(P.rptr[j + 1] - P.rptr[j]);
				b.cs_src = P.cs_src[j];
				b.pos = P.dense_pos[j];
			} else
				b.nr = -1;
			dense_blks.push_back(b);
			r_rec.dense_blk_loff.push_back(P.loff[k]);
		}
	}
	std::vector<char> covered(size_t(P.dense_dim), 0);
	for(size_t k = 0; k < dense_cols.size(); ++ k)
		std::fill(covered.begin() + dense_cols[k].pos, covered.begin() + dense_cols[k].pos + dense_cols[k].dj, char(1));
	for(int32_t q = 0; q < P.dense_dim; ++ q) {
		if(!covered[q])
			r_rec.gaps.push_back(q);
	}
	// the same as a byte per position (with the padding behind the last column: tile_zero writes the identity there
	// while it zeroes the diagonal tiles), and where every entry of the dense system's x goes in the solver's vectors
	// (the last launch of the substitution stores there: no scatter launch)
	r_rec.unit.assign(size_t(n_dense_pad), uint8_t(1));
	r_rec.dst.assign(size_t(n_dense_pad), longlong2{-1, -1});
	for(size_t k = 0; k < dense_cols.size(); ++ k) {
		for(int q = 0; q < dense_cols[k].dj; ++ q) {
			r_rec.unit[dense_cols[k].pos + q] = 0;
			r_rec.dst[dense_cols[k].pos + q] = longlong2{(long long)(dense_cols[k].cs_new + q), (long long)(dense_cols[k].cs_src + q)};
		}
	}
}

// ---- lane-per-task tables (simt_kernel.hip; the formats are described in sparse_kernels.h) ----

namespace {

enum { SIMT_MIN_GROUP = 1, SIMT_MAX_PROG = 4096, SIMT_MAX_TABLE_BYTES = 40960 }; // (rare shapes run with few busy lanes, beside the others: cheaper than a launch of their own)
struct TSimtTask { int32_t n_task; bool b_fits; uint64_t n_hash; std::vector<int32_t> prog, ops, ys; };
struct TSimtChunkJob { int32_t n_group; size_t n_first; int n_fields, n_bwd_fields; int64_t n_tab_off, n_bwd_tab_off; };

// the program of task t, its operands and its y columns in order of first use, whether it fits the kernel, the program's hash
// (op_index, y_index: per factor block and per column, all -1 when called and when left; touch, body: scratch)
// (p_cols: the columns the program walks, in elimination order -- a whole task's, or one segment's of a split task: below)
void Simt_Task_Program(const Plan &P, int32_t t, const int32_t *p_cols, int32_t n_cols, size_t W, int32_t *op_index, int32_t *y_index,
	std::vector<int32_t> &touch, std::vector<int32_t> &body, TSimtTask &tt)
{
	std::vector<int32_t> &prog = tt.prog;
	prog.assign(4, 0);
	tt.ops.clear();
	tt.ys.clear();
	tt.n_task = t;
	int32_t n_blocks = 0;
	bool b_fits = true;
	auto op_of = [&](int32_t n_blk) {
		if(op_index[n_blk] < 0) {
			op_index[n_blk] = int32_t(tt.ops.size());
			tt.ops.push_back(n_blk);
		}
		return op_index[n_blk];
	};
	for(int32_t i = 0; i < n_cols && b_fits; ++ i) {
		const int32_t j = p_cols[i];
		const int32_t nb = int32_t(P.lptr[j + 1] - P.lptr[j]), nr = int32_t(P.rptr[j + 1] - P.rptr[j]);
		prog.push_back(nb);
		prog.push_back(nr);
		const size_t n_touch_at = prog.size();
		prog.push_back(0); // number of distinct operands of the column, then their indices
		n_blocks += nb;
		touch.clear();
		body.clear();
		auto touch_op = [&](int32_t n_op) {
			if(std::find(touch.begin(), touch.end(), n_op) == touch.end())
				touch.push_back(n_op);
			return n_op;
		};
		for(int64_t e = P.rptr[j]; e < P.rptr[j + 1]; ++ e) {
			const int32_t n_blk = P.rblk[e], c = P.blk_col[n_blk];
			if(y_index[c] < 0) {
				y_index[c] = int32_t(tt.ys.size());
				tt.ys.push_back(c);
			}
			body.push_back(touch_op(op_of(n_blk)));
			body.push_back(y_index[c]);
		}
		for(int64_t k = P.lptr[j] + 1; k < P.lptr[j + 1]; ++ k) {
			body.push_back(int32_t(P.pptr[k + 1] - P.pptr[k]));
			for(int64_t e = P.pptr[k]; e < P.pptr[k + 1]; ++ e) {
				body.push_back(touch_op(op_of(P.pa[e])));
				body.push_back(touch_op(op_of(P.pb[e])));
			}
		}
		prog[n_touch_at] = int32_t(touch.size());
		prog.insert(prog.end(), touch.begin(), touch.end());
		prog.insert(prog.end(), body.begin(), body.end());
		b_fits = prog.size() <= SIMT_MAX_PROG;
	}
	for(size_t k = 0; k < tt.ops.size(); ++ k)
		op_index[tt.ops[k]] = -1;
	for(size_t k = 0; k < tt.ys.size(); ++ k)
		y_index[tt.ys[k]] = -1;
	// (round 6) behind the program proper: for every block below a diagonal, which of the task's columns its row is, or
	// -1 for a row outside the task -- what the backward kernel keeps x of in LDS.  Implied by the program (a block whose
	// row is column m of the task is a row entry of m), and part of the shape's key all the same
	for(int32_t i = 0; i < n_cols && b_fits; ++ i) {
		const int32_t j = p_cols[i];
		for(int64_t k = P.lptr[j] + 1; k < P.lptr[j + 1]; ++ k) {
			int32_t n_local = -1;
			for(int32_t i2 = i + 1; i2 < n_cols && n_local < 0; ++ i2) {
				if(p_cols[i2] == P.lrow[k])
					n_local = i2;
			}
			prog.push_back(n_local);
		}
	}
	prog[0] = n_cols;
	prog[1] = n_blocks;
	prog[2] = int32_t(tt.ops.size());
	prog[3] = int32_t(tt.ys.size());
	tt.b_fits = b_fits && size_t(4 * n_cols + n_blocks) + tt.ops.size() + tt.ys.size() <= SIMT_MAX_TABLE_BYTES / (8 * W); // (the table is staged in LDS)
	uint64_t h = 0x9e3779b97f4a7c15ull ^ prog.size();
	for(size_t k = 0; k < prog.size(); ++ k) {
		h ^= uint64_t(uint32_t(prog[k])) + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
		h *= 0xff51afd7ed558ccdull;
	}
	tt.n_hash = h;
}

// shapes: tasks of one hash whose programs are the same (compared in full against the shape's first task), in lexicographic
// order of their programs; the tasks that do not fit the kernel go to rest
void Group_Simt_Shapes(const std::vector<TSimtTask> &tasks_all, std::vector<int32_t> &rest, std::vector<std::vector<int32_t> > &groups) // groups: indices into tasks_all, ascending
{
	std::unordered_map<uint64_t, std::vector<int32_t> > by_hash; // hash -> the shapes that have it
	for(int32_t n_i = 0; n_i < int32_t(tasks_all.size()); ++ n_i) {
		const TSimtTask &tt = tasks_all[size_t(n_i)];
		if(!tt.b_fits) {
			rest.push_back(tt.n_task);
			continue;
		}
		std::vector<int32_t> &r_shapes = by_hash[tt.n_hash];
		int32_t n_group = -1;
		for(size_t k = 0; k < r_shapes.size() && n_group < 0; ++ k) {
			if(tasks_all[size_t(groups[size_t(r_shapes[k])][0])].prog == tt.prog)
				n_group = r_shapes[k];
		}
		if(n_group < 0) {
			n_group = int32_t(groups.size());
			groups.push_back(std::vector<int32_t>());
			r_shapes.push_back(n_group);
		}
		groups[size_t(n_group)].push_back(n_i);
	}
	std::sort(groups.begin(), groups.end(), [&](const std::vector<int32_t> &r_a, const std::vector<int32_t> &r_b) {
		return tasks_all[size_t(r_a[0])].prog < tasks_all[size_t(r_b[0])].prog; });
}

// where every shape's program, chunks and tables go: appends the stage's programs and chunks, counts the table sizes up,
// lists what Fill_Simt_Chunk_Tables() is to write; returns the stage's largest forward and backward LDS request
std::pair<int32_t, int32_t> Layout_Simt_Chunks(const Plan &P, size_t W, const std::vector<TSimtTask> &tasks_all,
	const std::vector<std::vector<int32_t> > &groups, SparseRecords &r_rec, size_t &n_tab_size, size_t &n_bwd_tab_size, std::vector<TSimtChunkJob> &jobs)
{
	int32_t n_stage_lds = 0, n_stage_bwd_lds = 0;
	for(size_t g = 0; g < groups.size(); ++ g) {
		const std::vector<int32_t> &r_members = groups[g];
		const std::vector<int32_t> &prog = tasks_all[size_t(r_members[0])].prog;
		if(r_members.size() < SIMT_MIN_GROUP) {
			for(int32_t n_i : r_members)
				r_rec.simt_rest.push_back(tasks_all[size_t(n_i)].n_task);
			continue;
		}
		const int32_t n_prog_off = int32_t(r_rec.simt_prog.size());
		r_rec.simt_prog.insert(r_rec.simt_prog.end(), prog.begin(), prog.end());
		const int n_cols = prog[0], n_blocks = prog[1], n_ops = prog[2], n_ys = prog[3];
		const int n_fields = 4 * n_cols + n_blocks + n_ops + n_ys;
		n_stage_lds = std::max(n_stage_lds, int32_t(n_fields * W * 8));
		// the shape's backward program: n_cols, blocks below the diagonals, nb per column
		const int32_t n_bwd_prog_off = int32_t(r_rec.simt_bwd_prog.size());
		const int n_bwd_fields = 3 * n_cols + (n_blocks - n_cols);
		n_stage_bwd_lds = std::max(n_stage_bwd_lds, int32_t((n_bwd_fields + n_cols * P.max_dim) * W * 8)); // (the table, and x of the task's own columns)
		r_rec.simt_bwd_prog.push_back(n_cols);
		r_rec.simt_bwd_prog.push_back(n_blocks - n_cols);
		{
			const TSimtTask &tt = tasks_all[size_t(r_members[0])];
			for(int64_t i = P.task_ptr[tt.n_task]; i < P.task_ptr[tt.n_task + 1]; ++ i)
				r_rec.simt_bwd_prog.push_back(int32_t(P.lptr[P.task_cols[i] + 1] - P.lptr[P.task_cols[i]]));
			// which of the task's columns every below-diagonal block's row is (the tail of the forward program: see there)
			r_rec.simt_bwd_prog.insert(r_rec.simt_bwd_prog.end(), prog.end() - (n_blocks - n_cols), prog.end());
		}
		for(size_t n_first = 0; n_first < r_members.size(); n_first += W) {
			const size_t n_in_chunk = std::min<size_t>(W, r_members.size() - n_first);
			TSimtChunk ch;
			ch.prog_off = n_prog_off;
			ch.n_tasks = int32_t(n_in_chunk);
			ch.tab_off = int64_t(n_tab_size);
			r_rec.simt_chunks.push_back(ch);
			TSimtChunk ch_bwd;
			ch_bwd.prog_off = n_bwd_prog_off;
			ch_bwd.n_tasks = int32_t(n_in_chunk);
			ch_bwd.tab_off = int64_t(n_bwd_tab_size);
			r_rec.simt_bwd_chunks.push_back(ch_bwd);
			TSimtChunkJob t_job = {int32_t(g), n_first, n_fields, n_bwd_fields, ch.tab_off, ch_bwd.tab_off};
			jobs.push_back(t_job);
			n_tab_size += size_t(n_fields) * W;
			n_bwd_tab_size += size_t(n_bwd_fields) * W;
		}
	}
	return std::make_pair(n_stage_lds, n_stage_bwd_lds);
}

// one lane of a forward table, [field][lane]: the fields of the columns p_cols (a whole task's, or a segment's), then of the
// operands and y columns of their program; returns the number of fields written
int Fill_Simt_Forward_Lane(const Plan &P, size_t W, int64_t *p_tab, int n_lane, const int32_t *p_cols, int32_t n_cols,
	const std::vector<int32_t> &r_ops, const std::vector<int32_t> &r_ys)
{
	int f = 0;
	for(int32_t i = 0; i < n_cols; ++ i) {
		const int32_t j = p_cols[i];
		p_tab[W * (f ++) + n_lane] = P.loff[P.lptr[j]];
		p_tab[W * (f ++) + n_lane] = P.linv_off[j];
		p_tab[W * (f ++) + n_lane] = P.cs_new[j];
		p_tab[W * (f ++) + n_lane] = P.cs_src[j];
	}
	for(int32_t i = 0; i < n_cols; ++ i) {
		const int32_t j = p_cols[i];
		for(int64_t k = P.lptr[j]; k < P.lptr[j + 1]; ++ k)
			p_tab[W * (f ++) + n_lane] = (P.asrc[k] < 0)? -1 : P.asrc[k] * 2 + P.atrans[k];
	}
	for(int32_t n_blk : r_ops)
		p_tab[W * (f ++) + n_lane] = P.loff[n_blk];
	for(int32_t c : r_ys)
		p_tab[W * (f ++) + n_lane] = P.cs_new[c];
	return f;
}

// the forward and the backward table of one chunk, [field][lane]
void Fill_Simt_Chunk_Tables(const Plan &P, size_t W, const std::vector<TSimtTask> &tasks_all, const std::vector<std::vector<int32_t> > &groups,
	const TSimtChunkJob &r_job, SparseRecords &r_rec)
{
	const std::vector<int32_t> &r_members = groups[size_t(r_job.n_group)];
	const size_t n_first = r_job.n_first, n_in_chunk = std::min<size_t>(W, r_members.size() - n_first);
	const int n_fields = r_job.n_fields, n_bwd_fields = r_job.n_bwd_fields;
	int64_t *p_tab = &r_rec.simt_tab[size_t(r_job.n_tab_off)];
	for(int n_lane = 0; n_lane < int(W); ++ n_lane) {
		const TSimtTask &tt = tasks_all[size_t(r_members[n_first + std::min<size_t>(n_lane, n_in_chunk - 1)])]; // spare lanes repeat the last task
		const int f = Fill_Simt_Forward_Lane(P, W, p_tab, n_lane, P.task_cols.data() + P.task_ptr[tt.n_task],
			int32_t(P.task_ptr[tt.n_task + 1] - P.task_ptr[tt.n_task]), tt.ops, tt.ys);
		if(f != n_fields)
			throw std::logic_error("lane-per-task tables: field count mismatch");
	}
	int64_t *p_bwd = &r_rec.simt_bwd_tab[size_t(r_job.n_bwd_tab_off)];
	for(int n_lane = 0; n_lane < int(W); ++ n_lane) {
		const TSimtTask &tt = tasks_all[size_t(r_members[n_first + std::min<size_t>(n_lane, n_in_chunk - 1)])];
		int f = 0;
		for(int64_t i = P.task_ptr[tt.n_task]; i < P.task_ptr[tt.n_task + 1]; ++ i) {
			const int32_t j = P.task_cols[i];
			p_bwd[W * (f ++) + n_lane] = P.loff[P.lptr[j]];
			p_bwd[W * (f ++) + n_lane] = P.cs_new[j];
			p_bwd[W * (f ++) + n_lane] = P.cs_src[j];
		}
		for(int64_t i = P.task_ptr[tt.n_task]; i < P.task_ptr[tt.n_task + 1]; ++ i) {
			const int32_t j = P.task_cols[i];
			for(int64_t k = P.lptr[j] + 1; k < P.lptr[j + 1]; ++ k) {
				if(P.loff[k] != P.loff[P.lptr[j]] + (k - P.lptr[j]) * int64_t(P.max_dim) * P.max_dim)
					throw std::logic_error("lane-per-task tables: the blocks of a column are not contiguous");
				p_bwd[W * (f ++) + n_lane] = P.cs_new[P.lrow[k]];
			}
		}
		if(f != n_bwd_fields)
			throw std::logic_error("lane-per-task tables: backward field count mismatch");
	}
}

} // anonymous namespace

void simt_task_parents(const Plan &P, int32_t t, std::vector<int32_t> &r_parent)
{
	const int32_t *p_cols = P.task_cols.data() + P.task_ptr[t];
	const int32_t n_cols = int32_t(P.task_ptr[t + 1] - P.task_ptr[t]);
	r_parent.assign(size_t(n_cols), -1);
	for(int32_t i = 0; i < n_cols; ++ i) { // the first of the task's columns among the rows below the diagonal
		const int32_t j = p_cols[i];
		for(int64_t k = P.lptr[j] + 1; k < P.lptr[j + 1]; ++ k) {
			for(int32_t i2 = i + 1; i2 < n_cols && (r_parent[size_t(i)] < 0 || i2 < r_parent[size_t(i)]); ++ i2) {
				if(p_cols[i2] == P.lrow[k])
					r_parent[size_t(i)] = i2;
			}
		}
	}
}

int32_t simt_task_segments(const std::vector<int32_t> &r_parent, TSimtSegments &r_seg)
{
	const int32_t n = int32_t(r_parent.size());
	std::vector<int32_t> n_children(size_t(n), 0);
	std::vector<char> b_join(size_t(n), 0);
	for(int32_t i = 0; i < n; ++ i) {
		if(r_parent[size_t(i)] >= 0)
			++ n_children[size_t(r_parent[size_t(i)])];
	}
	for(int32_t i = 0; i < n; ++ i) { // (ascending: a parent lies behind its children)
		b_join[size_t(i)] = b_join[size_t(i)] || n_children[size_t(i)] >= 2;
		if(b_join[size_t(i)] && r_parent[size_t(i)] >= 0)
			b_join[size_t(r_parent[size_t(i)])] = 1;
	}
	std::vector<std::vector<int32_t> > chains;
	for(int32_t i = 0; i < n; ++ i) {
		if(n_children[size_t(i)] != 0)
			continue;
		chains.push_back(std::vector<int32_t>());
		for(int32_t c = i; c >= 0 && !b_join[size_t(c)]; c = r_parent[size_t(c)])
			chains.back().push_back(c);
	}
	r_seg.n_tips = int32_t(chains.size());
	for(int k = 0; k < 3; ++ k)
		r_seg.seg[k].clear();
	std::stable_sort(chains.begin(), chains.end(), [](const std::vector<int32_t> &r_a, const std::vector<int32_t> &r_b) { return r_a.size() > r_b.size(); });
	for(size_t c = 0; c < chains.size(); ++ c) {
		std::vector<int32_t> &r_bin = r_seg.seg[(r_seg.seg[1].size() < r_seg.seg[0].size() && chains.size() > 1)? 1 : 0];
		r_bin.insert(r_bin.end(), chains[c].begin(), chains[c].end());
	}
	for(int32_t i = 0; i < n; ++ i) {
		if(b_join[size_t(i)])
			r_seg.seg[2].push_back(i);
	}
	std::sort(r_seg.seg[0].begin(), r_seg.seg[0].end());
	std::sort(r_seg.seg[1].begin(), r_seg.seg[1].end());
	return int32_t(std::max(r_seg.seg[0].size(), r_seg.seg[1].size()) + r_seg.seg[2].size());
}

namespace {

// an item of a stage's launch order in the two-wave forms: a chunk of split tasks, or two chunks of whole tasks
struct TSimtBranchItem {
	int32_t n_chain;          // the longest chain of columns a wave walks in it
	TSimtBranchGroup t_group; // the factor record
	char b_split;
	size_t n_group;           // split: the shape
	size_t n_chunk[2];        // the chunk of the split tasks, or the two chunks of whole tasks (size_t(-1): none), in simt_chunks / simt_bwd_chunks
};

// The same items in the same order as backward records (sparse_kernels.h: TSimtBwdBranchLaunch).  A segment's program is cut out
// of the whole task's backward program: n_cols, blocks below the diagonals, nb per column, per block which of the task's columns
// its row is (in the task's numbering: unchanged), and per column its place in the task.  Its table is the rows of the chunk's
// backward table that belong to its columns, [field][lane] as they are (spare lanes repeat the last task there already).  A chunk
// of whole tasks keeps its table and gets its program with the places 0 .. n_cols - 1 behind it.  Programs and tables go to
// bwd_prog and bwd_tab (build_simt_tables() puts them behind the chunks' own and moves the offsets); nothing the one-wave
// forms read is touched.  A stage whose LDS request -- three table regions and two x regions -- is beyond a plain launch's gets none.
void Build_Simt_Bwd_Branches(const Plan &P, size_t W, const std::vector<TSimtSegments> &segs, const std::vector<TSimtBranchItem> &items,
	SparseRecords &r_rec, TSimtBranchStage &r_stage, std::vector<int32_t> &bwd_prog, std::vector<int64_t> &bwd_tab, std::vector<char> &bwd_split)
{
	const size_t n_prog0 = bwd_prog.size(), n_tab0 = bwd_tab.size();
	std::map<std::pair<int32_t, int>, int32_t> prog_of; // (the whole task's program, segment or 3 for the whole task) -> where its program is
	std::vector<TSimtBranchGroup> records;
	std::vector<int32_t> blk0;
	size_t n_tab_region = 0;
	int32_t n_x_cols = 0;
	const TSimtChunk t_none = {0, 0, 0};
	for(size_t n_item = 0; n_item < items.size(); ++ n_item) {
		const TSimtBranchItem &r_item = items[n_item];
		TSimtBranchGroup t_record = {{t_none, t_none, t_none}};
		for(int n_half = 0; n_half < 2; ++ n_half) {
			if(r_item.n_chunk[n_half] == size_t(-1))
				continue;
			const TSimtChunk ch = r_rec.simt_bwd_chunks[r_item.n_chunk[n_half]];
			const int32_t *p_whole = &r_rec.simt_bwd_prog[size_t(ch.prog_off)];
			const int32_t n_cols = p_whole[0], n_below = p_whole[1];
			const int32_t *p_nb = p_whole + 2, *p_local = p_nb + n_cols;
			n_x_cols = std::max(n_x_cols, n_cols);
			r_stage.n_bwd_spare_chunks += size_t(ch.n_tasks) < W;
			blk0.assign(size_t(n_cols) + 1, 0); // the column's first block below the diagonal among the task's
			for(int32_t i = 0; i < n_cols; ++ i)
				blk0[size_t(i) + 1] = blk0[size_t(i)] + p_nb[i] - 1;
			for(int32_t i = 0; i < n_cols; ++ i) {
				int n_outside = 0;
				for(int32_t b = blk0[size_t(i)]; b < blk0[size_t(i) + 1]; ++ b)
					n_outside += p_local[b] < 0;
				r_stage.n_bwd_two_outside_columns += (n_outside >= 2)? ch.n_tasks : 0;
			}
			if(!r_item.b_split) {
				std::pair<std::map<std::pair<int32_t, int>, int32_t>::iterator, bool> t_at = prog_of.insert(std::make_pair(std::make_pair(ch.prog_off, 3), int32_t(bwd_prog.size())));
				if(t_at.second) {
					bwd_prog.insert(bwd_prog.end(), p_whole, p_whole + 2 + n_cols + n_below);
					for(int32_t i = 0; i < n_cols; ++ i)
						bwd_prog.push_back(i);
				}
				const TSimtChunk t_seg = {t_at.first->second, ch.n_tasks, ch.tab_off};
				t_record.seg[n_half] = t_seg;
				n_tab_region = std::max(n_tab_region, size_t(3 * n_cols + n_below) * W);
				continue;
			}
			const TSimtSegments &r_segs = segs[r_item.n_group];
			r_stage.n_bwd_tip3_tasks += (r_segs.n_tips >= 3)? ch.n_tasks : 0;
			for(int k = 0; k < 3; ++ k) {
				const std::vector<int32_t> &r_cols = r_segs.seg[k]; // (columns of the task, ascending)
				if(r_cols.empty())
					continue;
				int32_t n_seg_below = 0;
				for(int32_t c : r_cols) {
					n_seg_below += p_nb[c] - 1;
					r_stage.n_bwd_long_columns += (p_nb[c] > int32_t(SIMT_BWD_AHEAD) + 1)? ch.n_tasks : 0;
				}
				std::pair<std::map<std::pair<int32_t, int>, int32_t>::iterator, bool> t_at = prog_of.insert(std::make_pair(std::make_pair(ch.prog_off, k), int32_t(bwd_prog.size())));
				if(t_at.second) {
					bwd_prog.push_back(int32_t(r_cols.size()));
					bwd_prog.push_back(n_seg_below);
					for(int32_t c : r_cols)
						bwd_prog.push_back(p_nb[c]);
					for(int32_t c : r_cols)
						bwd_prog.insert(bwd_prog.end(), p_local + blk0[size_t(c)], p_local + blk0[size_t(c) + 1]);
					bwd_prog.insert(bwd_prog.end(), r_cols.begin(), r_cols.end());
				}
				const TSimtChunk t_seg = {t_at.first->second, ch.n_tasks, int64_t(bwd_tab.size())};
				t_record.seg[k] = t_seg;
				const int64_t *p_tab = &r_rec.simt_bwd_tab[size_t(ch.tab_off)];
				for(int32_t c : r_cols) // per column: its first factor block, its place in the workspace and in the caller's vector
					bwd_tab.insert(bwd_tab.end(), p_tab + size_t(3 * c) * W, p_tab + size_t(3 * c + 3) * W);
				for(int32_t c : r_cols) // per block below a diagonal: its row's place in the workspace
					bwd_tab.insert(bwd_tab.end(), p_tab + size_t(3 * n_cols + blk0[size_t(c)]) * W, p_tab + size_t(3 * n_cols + blk0[size_t(c) + 1]) * W);
				n_tab_region = std::max(n_tab_region, (3 * r_cols.size() + size_t(n_seg_below)) * W);
			}
		}
		records.push_back(t_record);
	}
	const size_t n_x_region = size_t(n_x_cols) * size_t(P.max_dim) * W;
	const size_t n_lds_bytes = (3 * n_tab_region + 2 * n_x_region) * 8;
	if(n_lds_bytes > 64 * 1024) { // (beyond a plain launch's LDS: the stage keeps the one-wave backward forms)
		bwd_prog.resize(n_prog0);
		bwd_tab.resize(n_tab0);
		r_stage.n_bwd_tip3_tasks = r_stage.n_bwd_long_columns = r_stage.n_bwd_two_outside_columns = r_stage.n_bwd_spare_chunks = 0;
		return;
	}
	r_stage.n_bwd_first = int32_t(r_rec.simt_bwd_br_groups.size());
	r_stage.n_bwd_groups = int32_t(records.size());
	r_stage.n_bwd_tab_region = int32_t(n_tab_region);
	r_stage.n_bwd_x_region = int32_t(n_x_region);
	r_stage.n_bwd_lds_bytes = int32_t(n_lds_bytes);
	r_rec.simt_bwd_br_groups.insert(r_rec.simt_bwd_br_groups.end(), records.begin(), records.end());
	for(size_t n_item = 0; n_item < items.size(); ++ n_item)
		bwd_split.push_back(items[n_item].b_split);
}

// The workgroup records of one stage for the two-wave factor form (sparse_kernels.h: TSimtBranchGroup).  Shapes stay grouped by
// the whole task's program, so a chunk of split tasks has one program per segment, shared by its lanes; the segments' programs
// and tables go to br_prog and br_tab (build_simt_tables() puts them behind the chunks' own and moves the offsets), the
// chunks of whole tasks are named as they are.  b_split_all: every shape with two bins splits (the development knob at 1: how
// small systems reach the form); otherwise the shapes with more columns than T* do, since splitting others would not shorten
// the launch -- and a stage where none does gets no records.
// n_chunk0: the stage's first chunk; jobs: one per chunk of the stage, in the chunks' order
void Build_Simt_Branches(const Plan &P, size_t W, bool b_split_all, int32_t n_stage_tasks, const std::vector<TSimtTask> &tasks_all,
	const std::vector<std::vector<int32_t> > &groups, const std::vector<TSimtChunkJob> &jobs, size_t n_chunk0, raw_vector<int32_t> &index_pool,
	SparseRecords &r_rec, TSimtBranchStage &r_stage, std::vector<int32_t> &br_prog, raw_vector<int64_t> &br_tab, std::vector<char> &br_split,
	std::vector<int32_t> &bwd_br_prog, std::vector<int64_t> &bwd_br_tab, std::vector<char> &bwd_br_split)
{
	r_stage = TSimtBranchStage();
	r_stage.n_first = int32_t(r_rec.simt_br_groups.size());
	r_stage.n_stage_tasks = n_stage_tasks;
	// 1. the segments of every shape, T*, which shapes split
	std::vector<TSimtSegments> segs(groups.size());
	std::vector<int32_t> chain(groups.size(), 0), parent;
	for(size_t g = 0; g < groups.size(); ++ g) {
		const TSimtTask &tt = tasks_all[size_t(groups[g][0])];
		simt_task_parents(P, tt.n_task, parent);
		chain[g] = simt_task_segments(parent, segs[g]);
		const int32_t n_cols = int32_t(parent.size());
		if(segs[g].seg[1].empty())
			chain[g] = n_cols;
		r_stage.n_tstar = std::max(r_stage.n_tstar, std::min(n_cols, chain[g]));
		r_stage.n_longest_task = std::max(r_stage.n_longest_task, n_cols);
	}
	std::vector<char> split(groups.size(), 0);
	bool b_any_split = false;
	for(size_t g = 0; g < groups.size(); ++ g) {
		const int32_t n_cols = tasks_all[size_t(groups[g][0])].prog[0];
		split[g] = !segs[g].seg[1].empty() && chain[g] < n_cols && (b_split_all || n_cols > r_stage.n_tstar);
		b_any_split = b_any_split || split[g];
	}
	if(!b_any_split && !b_split_all)
		return;
	// 2. the segments' programs, from the first task of every split shape.  Tasks of one program differ in nothing but where their
	// blocks live, so a segment's operand (or y column) is the same entry of the whole task's list in every task of the shape: the
	// other tasks' tables are filled through that map, and no program but the first task's is built
	std::vector<TSimtTask> seg_tasks(groups.size() * 3);
	std::vector<std::vector<int32_t> > seg_op_map(groups.size() * 3), seg_y_map(groups.size() * 3);
	{
		int32_t *op_index = &index_pool[0], *y_index = op_index + P.lrow.size(); // (all -1: as the programs' pass left them)
		std::vector<int32_t> touch, body, cols;
		for(size_t g = 0; g < groups.size(); ++ g) {
			if(!split[g])
				continue;
			const TSimtTask &r_first = tasks_all[size_t(groups[g][0])];
			for(size_t k = 0; k < 3; ++ k) {
				const std::vector<int32_t> &r_local = segs[g].seg[k];
				cols.resize(r_local.size());
				for(size_t i = 0; i < r_local.size(); ++ i)
					cols[i] = P.task_cols[size_t(P.task_ptr[r_first.n_task] + r_local[i])];
				TSimtTask &r_seg = seg_tasks[g * 3 + k];
				Simt_Task_Program(P, r_first.n_task, cols.data(), int32_t(cols.size()), W, op_index, y_index, touch, body, r_seg);
				for(int32_t n_blk : r_seg.ops) {
					const size_t n_at = size_t(std::find(r_first.ops.begin(), r_first.ops.end(), n_blk) - r_first.ops.begin());
					if(n_at == r_first.ops.size())
						throw std::logic_error("lane-per-task segments: an operand the whole task does not have");
					seg_op_map[g * 3 + k].push_back(int32_t(n_at));
				}
				for(int32_t c : r_seg.ys) {
					const size_t n_at = size_t(std::find(r_first.ys.begin(), r_first.ys.end(), c) - r_first.ys.begin());
					if(n_at == r_first.ys.size())
						throw std::logic_error("lane-per-task segments: a y column the whole task does not have");
					seg_y_map[g * 3 + k].push_back(int32_t(n_at));
				}
			}
		}
	}
	// 3. layout: a program per segment of a split shape, a table per segment of its chunks; the records
	typedef TSimtBranchItem TItem;
	struct TSegJob { size_t n_group, n_first; int n_seg, n_fields; int64_t n_tab_off; };
	std::vector<TItem> items;
	std::vector<std::pair<int32_t, size_t> > whole; // columns, chunk
	std::vector<TSegJob> seg_jobs;
	std::map<std::pair<int32_t, int32_t>, int32_t> split_by;
	int32_t n_region_bytes = 0;
	const TSimtChunk t_none = {0, 0, 0};
	for(size_t n_job = 0; n_job < jobs.size(); ) {
		const size_t g = size_t(jobs[n_job].n_group);
		const int32_t n_cols = tasks_all[size_t(groups[g][0])].prog[0];
		if(!split[g]) {
			for(; n_job < jobs.size() && size_t(jobs[n_job].n_group) == g; ++ n_job) {
				whole.push_back(std::make_pair(n_cols, n_chunk0 + n_job));
				n_region_bytes = std::max(n_region_bytes, int32_t(jobs[n_job].n_fields * W * 8));
			}
			continue;
		}
		int32_t n_seg_prog_off[3] = {0, 0, 0};
		int n_seg_fields[3] = {0, 0, 0};
		for(size_t k = 0; k < 3; ++ k) {
			const std::vector<int32_t> &prog = seg_tasks[g * 3 + k].prog;
			n_seg_prog_off[k] = int32_t(br_prog.size());
			n_seg_fields[k] = 4 * prog[0] + prog[1] + prog[2] + prog[3];
			if(prog[0] > 0) {
				br_prog.insert(br_prog.end(), prog.begin(), prog.end());
				n_region_bytes = std::max(n_region_bytes, int32_t(n_seg_fields[k] * W * 8));
			}
		}
		const int32_t n_bin = int32_t(std::max(segs[g].seg[0].size(), segs[g].seg[1].size())), n_joins = int32_t(segs[g].seg[2].size());
		split_by[std::make_pair(n_bin, n_joins)] += int32_t(groups[g].size());
		r_stage.n_split_tasks += int32_t(groups[g].size());
		for(; n_job < jobs.size() && size_t(jobs[n_job].n_group) == g; ++ n_job) {
			const size_t n_first = jobs[n_job].n_first;
			TItem t_item;
			t_item.n_chain = chain[g];
			t_item.b_split = 1;
			t_item.n_group = g;
			t_item.n_chunk[0] = n_chunk0 + n_job;
			t_item.n_chunk[1] = size_t(-1);
			for(size_t k = 0; k < 3; ++ k) {
				TSimtChunk &ch = t_item.t_group.seg[k];
				ch = t_none;
				if(!n_seg_fields[k])
					continue;
				ch.prog_off = n_seg_prog_off[k];
				ch.n_tasks = int32_t(std::min<size_t>(W, groups[g].size() - n_first));
				ch.tab_off = int64_t(br_tab.size());
				const TSegJob t_seg_job = {g, n_first, int(k), n_seg_fields[k], ch.tab_off};
				seg_jobs.push_back(t_seg_job);
				br_tab.resize(br_tab.size() + size_t(n_seg_fields[k]) * W);
			}
			items.push_back(t_item);
			++ r_stage.n_split_chunks;
		}
	}
	Parallel_Ranges(int64_t(seg_jobs.size()), 32, [&](int64_t n_b, int64_t n_e) {
		std::vector<int32_t> cols, ops, ys;
		for(int64_t n_j = n_b; n_j < n_e; ++ n_j) {
			const TSegJob &r_job = seg_jobs[size_t(n_j)];
			const std::vector<int32_t> &r_local = segs[r_job.n_group].seg[r_job.n_seg], &r_members = groups[r_job.n_group];
			const std::vector<int32_t> &r_op_map = seg_op_map[r_job.n_group * 3 + size_t(r_job.n_seg)], &r_y_map = seg_y_map[r_job.n_group * 3 + size_t(r_job.n_seg)];
			const size_t n_in_chunk = std::min<size_t>(W, r_members.size() - r_job.n_first);
			cols.resize(r_local.size());
			ops.resize(r_op_map.size());
			ys.resize(r_y_map.size());
			for(int n_lane = 0; n_lane < int(W); ++ n_lane) {
				const TSimtTask &tt = tasks_all[size_t(r_members[r_job.n_first + std::min<size_t>(size_t(n_lane), n_in_chunk - 1)])]; // spare lanes repeat the last task
				for(size_t i = 0; i < r_local.size(); ++ i)
					cols[i] = P.task_cols[size_t(P.task_ptr[tt.n_task] + r_local[i])];
				for(size_t i = 0; i < r_op_map.size(); ++ i)
					ops[i] = tt.ops[size_t(r_op_map[i])];
				for(size_t i = 0; i < r_y_map.size(); ++ i)
					ys[i] = tt.ys[size_t(r_y_map[i])];
				if(Fill_Simt_Forward_Lane(P, W, &br_tab[size_t(r_job.n_tab_off)], n_lane, cols.data(), int32_t(cols.size()), ops, ys) != r_job.n_fields)
					throw std::logic_error("lane-per-task segments: field count mismatch");
			}
		}
	}, 8);
	// chunks of whole tasks two to a record, neighbours in length; the records by their chain, longest first (as Sort_Launch_Order())
	std::stable_sort(whole.begin(), whole.end(), [](const std::pair<int32_t, size_t> &r_a, const std::pair<int32_t, size_t> &r_b) { return r_a.first > r_b.first; });
	for(size_t i = 0; i < whole.size(); i += 2) {
		TItem t_item;
		t_item.n_chain = whole[i].first;
		t_item.b_split = 0;
		t_item.n_group = size_t(-1);
		t_item.n_chunk[0] = whole[i].second;
		t_item.n_chunk[1] = (i + 1 < whole.size())? whole[i + 1].second : size_t(-1);
		t_item.t_group.seg[0] = r_rec.simt_chunks[whole[i].second];
		t_item.t_group.seg[1] = (i + 1 < whole.size())? r_rec.simt_chunks[whole[i + 1].second] : t_none;
		t_item.t_group.seg[2] = t_none;
		items.push_back(t_item);
	}
	r_stage.n_whole_chunks = int32_t(whole.size());
	std::stable_sort(items.begin(), items.end(), [](const TItem &r_a, const TItem &r_b) { return r_a.n_chain > r_b.n_chain; });
	if(2 * int64_t(n_region_bytes) > 64 * 1024) { // (beyond a plain launch's LDS: the stage keeps the one-wave forms; what went to br_prog and br_tab is not referred to)
		r_stage.n_split_tasks = r_stage.n_split_chunks = r_stage.n_whole_chunks = 0;
		return;
	}
	for(size_t i = 0; i < items.size(); ++ i) {
		r_rec.simt_br_groups.push_back(items[i].t_group);
		br_split.push_back(items[i].b_split);
		r_stage.n_longest_chain = std::max(r_stage.n_longest_chain, items[i].n_chain);
	}
	r_stage.n_groups = int32_t(items.size());
	r_stage.n_lds_bytes = 2 * n_region_bytes;
	Build_Simt_Bwd_Branches(P, W, segs, items, r_rec, r_stage, bwd_br_prog, bwd_br_tab, bwd_br_split);
	for(std::map<std::pair<int32_t, int32_t>, int32_t>::const_iterator p = split_by.begin(); p != split_by.end(); ++ p) {
		r_stage.split_by.push_back(p->first.first);
		r_stage.split_by.push_back(p->first.second);
		r_stage.split_by.push_back(p->second);
	}
}

} // anonymous namespace

// Sorts the tasks of the wide bottom stages by shape for the lane-per-task kernel.  A shape is the task's whole program --
// counts and operand indices, the operands numbered in order of first use -- so two tasks of one shape differ in nothing
// but where their blocks live.  (No HIP call: runs on a thread of its own next to the rest of the analysis; sparse_setup.hip
// sends what it built.)
void build_simt_tables(const Plan &P, const SparseRecordOptions &t_opt, SparseRecords &r_rec, SparseLaunchLists &r_lists)
{
	r_lists.simt_chunk_ptr.clear();
	r_lists.simt_rest_ptr.clear();
	r_lists.simt_lds_bytes.clear();
	r_rec.simt_chunks.clear(); r_rec.simt_prog.clear(); r_rec.simt_tab.clear(); r_rec.simt_rest.clear();
	r_lists.simt_bwd_lds_bytes.clear();
	r_lists.simt_br.clear();
	r_rec.simt_br_groups.clear();
	r_rec.simt_bwd_br_groups.clear();
	r_rec.simt_bwd_chunks.clear(); r_rec.simt_bwd_prog.clear(); r_rec.simt_bwd_tab.clear();
	if(!t_opt.n_simt || !b_Package_Dim(P))
		return;
	// one lane per leaf task pays when there are enough tasks to fill waves with them: a small system (the reduced camera
	// system of 1000 cameras has 250 leaf tasks) is faster with a wave per task (0.49 -> 0.42 ms there)
	if(t_opt.n_simt < 0 && P.stage_ptr.size() > 1 && P.stage_ptr[1] - P.stage_ptr[0] < 2048)
		return;
	const int n_stages = int(P.stage_ptr.size()) - 1;
	std::vector<int32_t> &rest = r_rec.simt_rest;
	size_t n_tab_size = 0, n_bwd_tab_size = 0; // (the tables are laid out first and made in one piece after the layout of a stage: round 6 --
	// grown chunk by chunk, zero-filled and moved as they grew, they were most of the 5 ms the layout took at C3)
	// Round 6: the tasks' programs on several threads (a task's program depends on nothing but the plan), the shapes told
	// apart by a hash of the program with one full comparison per task against its shape's first member instead of a
	// std::map keyed by the programs (16 000 insertions of 200-word keys at C3), the tables of a shape's chunks on several
	// threads again.  Shapes, chunks and tables come out in the order the map gave them (programs in lexicographic order,
	// the tasks of a shape ascending).
	r_lists.simt_chunk_ptr.push_back(0);
	r_lists.simt_rest_ptr.push_back(0);
	const size_t W = size_t(t_opt.n_simt_width);
	// the workgroup records of the two-wave factor form, where the fetch-ahead form exists for the stage (block size 6, two lanes
	// a task: widths 16 and 32).  Development aid SLAMPP_HIP_DEV_SIMT_FACTOR_BRANCHES (plan.h): 0 = none, 1 = every shape with two
	// bins splits; the launches read the knob again (simt_kernel.hip).  The same items become the records of the two-wave backward
	// form, with a knob of their own, SLAMPP_HIP_DEV_SIMT_BWD_BRANCHES: at 1 it too makes every shape with two bins split, and
	// the records are built even where the factor knob is 0
	const int n_branches_env = dev_knob("SLAMPP_HIP_DEV_SIMT_FACTOR_BRANCHES", -1), n_bwd_branches_env = dev_knob("SLAMPP_HIP_DEV_SIMT_BWD_BRANCHES", -1);
	const bool b_branches = (n_branches_env != 0 || n_bwd_branches_env == 1) && P.uniform_dim && P.max_dim == 6 && (W == 16 || W == 32);
	std::vector<int32_t> br_prog, bwd_br_prog;
	raw_vector<int64_t> br_tab; // (written in full by Build_Simt_Branches())
	std::vector<int64_t> bwd_br_tab;
	std::vector<char> br_split, bwd_br_split; // per record: its segments are in br_prog and br_tab
	for(int s = 0; s < r_lists.n_bottom_stages && s < n_stages && s < t_opt.n_simt_stages; ++ s) {
		const int32_t t0 = P.stage_ptr[s], n_stage_tasks = P.stage_ptr[s + 1] - P.stage_ptr[s];
		double t_simt_phase = wall_ms();
		auto Simt_Phase = [&](const char *p_s_name) { if(t_opt.b_timing) { const double t_ = wall_ms();
			fprintf(stderr, "[shapes] stage %d %-12s %8.2f ms\n", s, p_s_name, t_ - t_simt_phase); t_simt_phase = t_; } };
		std::vector<TSimtTask> tasks_all(size_t(std::max(n_stage_tasks, 0)));
		// (the threads' index arrays: made here, before the threads, and given back after them -- an array of megabytes made
		// and freed by a thread is an mmap and a munmap while a dozen other threads of the analysis run: see the panel packages)
		enum { SIMT_THREADS = 8 };
		raw_vector<int32_t> index_pool((P.lrow.size() + size_t(P.n)) * SIMT_THREADS); // (every thread fills its own slice)
		std::atomic<int> n_next_slice(0);
		Parallel_Ranges(n_stage_tasks, 512, [&](int64_t n_b, int64_t n_e) {
			const size_t n_slice = size_t(n_next_slice.fetch_add(1)) % SIMT_THREADS;
			int32_t *op_index = &index_pool[(P.lrow.size() + size_t(P.n)) * n_slice], *y_index = op_index + P.lrow.size();
			std::fill(op_index, op_index + P.lrow.size() + size_t(P.n), -1);
			std::vector<int32_t> touch, body;
			for(int64_t n_i = n_b; n_i < n_e; ++ n_i)
				Simt_Task_Program(P, t0 + int32_t(n_i), P.task_cols.data() + P.task_ptr[t0 + n_i], int32_t(P.task_ptr[t0 + n_i + 1] - P.task_ptr[t0 + n_i]), W,
					op_index, y_index, touch, body, tasks_all[size_t(n_i)]);
		}, 8);
		Simt_Phase("programs");
		std::vector<std::vector<int32_t> > groups;
		Group_Simt_Shapes(tasks_all, rest, groups);
		Simt_Phase("grouping");
		std::vector<TSimtChunkJob> jobs;
		const std::pair<int32_t, int32_t> t_stage_lds = Layout_Simt_Chunks(P, W, tasks_all, groups, r_rec, n_tab_size, n_bwd_tab_size, jobs);
		if(b_branches) { // (the segments' tables are at most the size of the tasks' own: room for them now, so that nothing is moved when they are put behind)
			r_rec.simt_tab.reserve(2 * n_tab_size);
			br_tab.reserve(n_tab_size);
		}
		r_rec.simt_tab.resize(n_tab_size); // (raw_vector: what was there stays, the new part is written in full below)
		r_rec.simt_bwd_tab.resize(n_bwd_tab_size);
		Simt_Phase("layout");
		Parallel_Ranges(int64_t(jobs.size()), 32, [&](int64_t n_b, int64_t n_e) {
			for(int64_t n_job = n_b; n_job < n_e; ++ n_job)
				Fill_Simt_Chunk_Tables(P, W, tasks_all, groups, jobs[size_t(n_job)], r_rec);
		}, 8);
		Simt_Phase("tables");
		r_lists.simt_br.push_back(TSimtBranchStage());
		if(b_branches) {
			Build_Simt_Branches(P, W, n_branches_env == 1 || n_bwd_branches_env == 1, n_stage_tasks, tasks_all, groups, jobs, r_rec.simt_chunks.size() - jobs.size(), index_pool,
				r_rec, r_lists.simt_br.back(), br_prog, br_tab, br_split, bwd_br_prog, bwd_br_tab, bwd_br_split);
			Simt_Phase("branches");
		}
		std::sort(rest.begin() + r_lists.simt_rest_ptr.back(), rest.end());
		r_lists.simt_chunk_ptr.push_back(int32_t(r_rec.simt_chunks.size()));
		r_lists.simt_rest_ptr.push_back(int32_t(rest.size()));
		r_lists.simt_lds_bytes.push_back(t_stage_lds.first);
		r_lists.simt_bwd_lds_bytes.push_back(t_stage_lds.second);
	}
	if(r_rec.simt_chunks.empty()) {
		r_lists.simt_chunk_ptr.clear();
		r_lists.simt_rest_ptr.clear();
	}
	if(r_rec.simt_br_groups.empty())
		r_lists.simt_br.clear();
	else { // the segments' programs and tables behind the chunks' own, which stay where they were
		const int32_t n_prog_base = int32_t(r_rec.simt_prog.size());
		const int64_t n_tab_base = int64_t(r_rec.simt_tab.size());
		r_rec.simt_prog.insert(r_rec.simt_prog.end(), br_prog.begin(), br_prog.end());
		r_rec.simt_tab.resize(size_t(n_tab_base) + br_tab.size());
		std::copy(br_tab.begin(), br_tab.end(), r_rec.simt_tab.begin() + n_tab_base);
		for(size_t i = 0; i < r_rec.simt_br_groups.size(); ++ i) {
			for(int k = 0; k < 3 && br_split[i]; ++ k) {
				TSimtChunk &ch = r_rec.simt_br_groups[i].seg[k];
				if(ch.n_tasks > 0) {
					ch.prog_off += n_prog_base;
					ch.tab_off += n_tab_base;
				}
			}
		}
	}
	if(!r_rec.simt_bwd_br_groups.empty()) { // the same for the backward records (a chunk of whole tasks keeps the table it has)
		const int32_t n_prog_base = int32_t(r_rec.simt_bwd_prog.size());
		const int64_t n_tab_base = int64_t(r_rec.simt_bwd_tab.size());
		r_rec.simt_bwd_prog.insert(r_rec.simt_bwd_prog.end(), bwd_br_prog.begin(), bwd_br_prog.end());
		r_rec.simt_bwd_tab.resize(size_t(n_tab_base) + bwd_br_tab.size());
		std::copy(bwd_br_tab.begin(), bwd_br_tab.end(), r_rec.simt_bwd_tab.begin() + n_tab_base);
		for(size_t i = 0; i < r_rec.simt_bwd_br_groups.size(); ++ i) {
			for(int k = 0; k < 3; ++ k) {
				TSimtChunk &ch = r_rec.simt_bwd_br_groups[i].seg[k];
				if(ch.n_tasks > 0) {
					ch.prog_off += n_prog_base;
					if(bwd_br_split[i])
						ch.tab_off += n_tab_base;
				}
			}
		}
	}
}

} // namespace slampp
