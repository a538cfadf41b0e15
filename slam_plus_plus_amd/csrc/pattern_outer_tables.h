// pattern_outer_tables.h -- host lookup tables of the outer product on Lambda's block pattern (pattern_outer.hip): where
// every stored block begins in the packed values, which scalar rows of the two vectors it pairs, and the first block of
// every chunk of pattern_outer_CHUNK consecutive packed values.
// Depends on the standard library only, no device calls: compiled on its own under the sanitizers
// (tests/pattern_outer_tables_driver.cpp).
#pragma once
#include <stdint.h>
#include <vector>

namespace slampp {

// packed values per chunk: what one wave writes with one 16-byte store per lane
enum { pattern_outer_CHUNK = 128 };

struct PatternOuterTables {
	std::vector<int64_t> boff;   // [n_blocks + 1] offset of every stored block in the packed values; the last entry is n_values
	std::vector<int32_t> row0;   // [n_blocks] first scalar row of the block's block row r
	std::vector<int32_t> col0;   // [n_blocks] first scalar row of its block column c (row0 == col0: a diagonal block)
	std::vector<int32_t> rows;   // [n_blocks] d_r: the block is d_r x d_c, column-major
	std::vector<int32_t> chunk;  // [n_chunks + 1] block that holds packed value q * pattern_outer_CHUNK; the last entry is n_blocks - 1
	int64_t n_values = 0, n_chunks = 0;
	int n_bisect_steps = 0;      // halvings that find a block between two chunk entries: 2^steps >= the most blocks a chunk touches
};

// One pass over the blocks (block-CSC of the upper triangle as slampp_hip_set_structure checked it: positive widths,
// block rows inside the upper triangle).  Throws std::domain_error where an index does not fit its 32 bits (2^31 scalars
// or blocks, or as many values in one block).  A structure without blocks gives empty tables (n_values = 0).
void pattern_outer_build_tables(int64_t n_bcols, const std::vector<int64_t> &r_cumsum, const std::vector<int64_t> &r_bcol_ptr,
	const std::vector<int32_t> &r_brow, PatternOuterTables &r_out);

} // namespace slampp
