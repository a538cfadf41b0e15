// schur_tile_tables.h -- host tables of the landmark-major assembly of the reduced camera system (schur_tiles.hip) and the
// contribution lists of schur.hip: what the BA analysis lays out for the kernels, from the structure alone.  Host code only:
// no HIP call, nothing of the handle (solver.h); schur_tiles.hip and schur_setup.hip run these builders and upload what they
// made, tests/schur_tile_tables_driver.cpp runs them on the CPU under sanitizers.
#pragma once
#include "plan.h"
#include "host_pool.h"
#include "host_threads.h"

#include <algorithm>
#include <cstdint>
#include <memory>
#include <vector>

namespace slampp {

enum { SCHUR_TILE_SLOTS = 64, SCHUR_TILE_MAX_POINTS = 64 };

struct TRunJob { // one wave of the run kernel
	int32_t n_first, n_points; // landmarks [n_first, n_first + n_points) of the run list
	int32_t n_k, n_rb, n_cb;   // cameras of the run's landmarks; observation blocks of the rows and of the columns
	int32_t n_pad;
	int64_t n_pbase;           // first partial block
};

constexpr int tile_max_k(int n_cap)
{
	int k = 1;
	while((k + 1) * (k + 2) / 2 <= n_cap)
		++ k;
	return k;
}

// What a launch takes from the analysis' counts, in one place each: tiles_enqueue_t (schur_tiles.hip) launches by these, and
// schur_tile_report reports them (SLAMPP_HIP_PLAN_TIMING: the "[schur report]" lines tests/test_schur_variants_gpu.py reads)
// -- the report cannot say one thing and the launch do another.
// Quads of landmarks wherever a job stages a multiple of four landmarks at a time: all but the off-diagonal jobs of three
// and four tiles a side, which stage two.  (Those with four staged and quads need 286 registers, one wave per SIMD instead
// of two: Venice-like C4 1.513 against 1.502 ms, not kept.  Quads also for the diagonal jobs of three and four tiles a side,
// four landmarks staged at a time: Venice-like C4 1.545 -> 1.486 ms.)
inline bool run_launch_quad(int n_tiles_a_side, bool b_diag)
{
	const bool b_quad = !dev_knob_set("SLAMPP_HIP_DEV_NO_QUAD_RUNS"); // (development: the one-landmark-per-step form, for A/B timing)
	const bool b_quad_wide = !dev_knob_set("SLAMPP_HIP_DEV_NO_QUAD_WIDE"); // (development: no quads for the diagonal jobs of three and four tiles a side)
	return (n_tiles_a_side <= 2 || (b_diag && b_quad_wide)) && b_quad;
}

// 64-lane loads that fetch the blocks of a tile launch's largest landmark (NL of schur_tile_kernel): at most what the
// largest landmark a tile takes needs
inline int tile_launch_loads(int DC, int DP, int64_t n_max_k)
{
	const int BLK = DC * DP, NL_MAX = (tile_max_k(SCHUR_TILE_SLOTS) * BLK + 63) / 64;
	const int64_t n_loads = (n_max_k * BLK + 63) / 64;
	return int(std::max<int64_t>(1, std::min<int64_t>(n_loads, std::min(4, NL_MAX))));
}

// the BA structure an analysis reads: block columns [0, nc) are cameras, [nc, nc + np) landmarks; the column of landmark pt
// holds the rows brow[ptr[nc + pt] ..] of the cameras that see it, ascending, and its own diagonal block last
struct SchurStructure {
	int DC, DP;
	int64_t nc, np;
	const int64_t *ptr;
	const int32_t *brow;
	int64_t n_ablocks; // camera-camera blocks in front of the values (ptr[nc])
	int64_t n_K(int64_t pt) const { return ptr[nc + pt + 1] - ptr[nc + pt] - 1; } // cameras of landmark pt
	const int32_t *p_Cams(int64_t pt) const { return brow + ptr[nc + pt]; }
	int64_t n_First_Obs(int64_t pt) const { return ptr[nc + pt] - ptr[nc] - pt; } // its first observation
};

// the run tables: what the run kernel reads, apart from run_rec.  Shared: the thread that uploads them beside the rest of
// the analysis owns what it reads (schur_tiles.h: TRunUpload)
struct SchurRunTables {
	raw_vector<TRunJob> jobs;
	raw_vector<int32_t> run_lm, run_k; // landmarks of the runs, piece after piece; their own number of observations
};

struct TTileRun { // the tiles of one contiguous piece of the sorted landmark order
	std::vector<int32_t> tile_size, tile_lm;  // landmarks per tile; the landmarks
	std::vector<int32_t> tile_slots;          // blocks per tile
	std::vector<int64_t> slot_key;            // their keys, tile after tile
	std::vector<uint8_t> lm_slot;             // slots of the landmarks' pairs, landmark after landmark
	std::vector<int32_t> rejected;            // landmarks left to the lists
};

// the host arrays and counts of one tile analysis, until they are on the device (the role SparseRecords plays for the
// sparse path).  Filled in three steps, in this order: schur_tile_routes, schur_tile_reduce_lists, schur_tile_xlists.
struct SchurTileTables {
	// ---- schur_tile_routes: which landmark goes where ----
	const char *p_s_keep_rule = 0; // the rule that left everything to the contribution lists, null: the tables are in use
	std::shared_ptr<SchurRunTables> p_runs;
	int64_t n_run_jobs[5][2][2] = {}, n_run_job_first[5][2][2] = {}; // jobs by (16-line tiles per side, row block == column block, some landmarks end before the run's list)
	raw_vector<int64_t> slot_key;       // the block of S (col * nc + row) of every partial block: runs first, then tiles
	raw_vector<uint8_t> handled;        // [np] landmarks that do not go through the contribution lists (routes: those in runs; reduce lists: and those in tiles)
	std::vector<TTileRun> tile_pieces;  // the tiles as the cutter left them, piece after piece of the tile order
	int64_t n_all_pairs = 0, n_run_pairs = 0, n_run_slots = 0, n_run_points = 0, n_prefix_points = 0;
	int64_t n_tiles = 0, n_slots = 0, n_tile_points = 0, n_list_points = 0, n_tile_pairs = 0 /* runs' and tiles' */, n_max_slots = 0, n_max_k = 0;
	CTrashList trash; // the big work arrays of the passes, freed beside the uploads (host_pool.h)
	// ---- schur_tile_reduce_lists ----
	std::vector<int32_t> tile_ptr, tile_lm;       // [n_tiles + 1] into tile_lm; landmarks of the tiles, in processing order
	std::vector<int64_t> tile_slot_ptr, pair_ptr; // [n_tiles + 1] the tile's partial blocks; [np + 1] into lm_slot
	std::vector<uint8_t> lm_slot;                 // tile-local slot of every camera pair of every landmark, pair (a <= b) at b (b + 1) / 2 + a
	std::vector<int64_t> rb_ptr;                  // [n_rb + 1] partial blocks of every block of S that has some
	std::vector<int32_t> rb_part, rb_sb;
	int64_t n_rb = 0;
	// ---- schur_tile_xlists: the landmarks left to the contribution lists ----
	std::vector<int32_t> xpoints, xsb_map, xent_a, xcam_obs;
	std::vector<int64_t> xsb_ptr, xent_uoff, xcam_ptr;
	// ---- the "[schur tiles] phase ms" lines (SLAMPP_HIP_PLAN_TIMING) ----
	bool b_timing = false;
	double t_phase = 0;
	void Phase(const char *p_s_name);
	// (between the steps: key -> block of S, made by schur_tile_reduce_lists)
	std::vector<int64_t> sb_keys;
	std::vector<int32_t> key_sb;
	size_t n_Block_Of(int64_t n_key) const; // sb_keys.size(): none
};

// n_mode: -1 = runs of at least four landmarks, tiles where landmarks share blocks, both only if together they take half of
// the contributions; 1 = runs of two and every tile that can be formed; 2 = tiles only; 3 = runs only, of any length.
// Returns whether the tables are in use (else T.p_s_keep_rule names the rule, and the "[schur report]" says so).
bool schur_tile_routes(SchurTileTables &T, int n_mode, const SchurStructure &r_s);
// the counts of the launches, the report, the tile kernel's tables and the partial blocks of every block of S
// (sb_row / sb_col: the blocks of S sorted by (col, row), as the contribution lists have them)
void schur_tile_reduce_lists(SchurTileTables &T, const SchurStructure &r_s, const std::vector<int32_t> &sb_row, const std::vector<int32_t> &sb_col);
void schur_tile_xlists(SchurTileTables &T, const SchurStructure &r_s);
// offset of the first U block of landmarks p_lm[0 .. n) in the values, which hold [U .. U | C] per landmark
void schur_run_records(int64_t *p_rec, const int32_t *p_lm, int64_t n, const SchurStructure &r_s);
// the "[schur] of N landmarks" and "[schur report]" lines of an analysis whose tables are in use
void schur_tile_report(const SchurTileTables &T, const SchurStructure &r_s);

// ---- contributions to S grouped by block (row = camera of b, col = camera of a, a <= b within a landmark) ----
// obs_cam: the camera of every observation, landmark after landmark

// the blocks of S that exist, sorted by (col, row): a bit per camera pair (nc * nc <= 2^26)
void schur_blocks_from_bitmap(std::vector<int32_t> &sb_row, std::vector<int32_t> &sb_col, const SchurStructure &r_s,
	const raw_vector<int32_t> &obs_cam, int n_workers);
// the lists of every block by a counting sort over the dense key space; sb_row / sb_col from schur_blocks_from_bitmap
void schur_lists_by_counting(std::vector<int64_t> &sb_ptr, raw_vector<int32_t> &ent_a, raw_vector<int64_t> &ent_uoff,
	const SchurStructure &r_s, const raw_vector<int32_t> &obs_cam, int64_t n_entries, size_t n_sblocks, int n_workers);
// blocks and lists by a comparison sort on (key, a, b): beyond the dense key space
void schur_lists_by_sorting(std::vector<int64_t> &sb_ptr, std::vector<int32_t> &sb_row, std::vector<int32_t> &sb_col,
	raw_vector<int32_t> &ent_a, raw_vector<int64_t> &ent_uoff, const SchurStructure &r_s, const raw_vector<int32_t> &obs_cam,
	const raw_vector<int32_t> &obs_pt, int64_t n_entries);

} // namespace slampp
