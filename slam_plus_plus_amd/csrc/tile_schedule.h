// tile_schedule.h -- the tables of the dense top's tile schedule (dense_chol.h: CTileSchedule), host only: no HIP
// dependency, so that a plain C++ program can build them and a CPU replay can check them (tests/tile_replay.py)
#pragma once
#include <vector>

namespace slampp {

struct TTileRec4 { int x, y, z, w; }; // (the layout of the device's int4)
struct TTileRec2 { int x, y; };

struct TTileTables {
	int n_tiles = 0, n_levels = 0;
	std::vector<int> height;           // [n_tiles] height of every tile column in the tile elimination tree
	std::vector<int> potrf;            // tile columns, level by level
	std::vector<TTileRec4> trsm;       // (row tile, column tile, 1 = the workgroup also updates the diagonal tile of its row, -)
	std::vector<TTileRec4> tgt;        // (row tile, column tile, first source, one past the last source)
	std::vector<int> src;              // source tile columns of the targets and of the riders
	std::vector<TTileRec4> riders;     // (row tile, column tile, first source, one past the last source)
	std::vector<TTileRec4> back_diag;  // (tile column k, its ancestor of height + 1 or -1, 1 = z_k is still y, -)
	std::vector<TTileRec4> back_carry; // (source tile column j, target tile column k, 1 = z_k is still y, -)
	std::vector<int> level_potrf_ptr, level_trsm_ptr, level_tgt_ptr; // [n_levels + 1] each
	std::vector<int> level_urgent_end; // [n_levels]
	std::vector<int> rider_ptr;        // [n_levels + 1]
	std::vector<int> back_diag_ptr, back_carry_ptr; // [n_levels + 1] each, by launch
};

// Everything CTileSchedule::Build() uploads.  r_nonzero: n_tiles x n_tiles flags, column-major, lower triangle; the
// diagonal and the last tile row are taken as nonzero.  n_rider_chunk: sources of one target that a launch takes ahead
// of the target's deadline; n_rider_budget: source tiles a launch takes ahead of their deadline.  Returns false where
// the tables contradict themselves (cannot happen); r_tables is then incomplete.
bool tile_schedule_tables(int n_tiles, const std::vector<char> &r_nonzero, int n_rider_chunk, int n_rider_budget,
	TTileTables &r_tables);

} // namespace slampp
