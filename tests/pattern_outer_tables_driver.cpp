// Test infrastructure (tests/test_torch_solve_host.py): the host lookup tables of the outer product on Lambda's pattern
// (csrc/pattern_outer_tables.cpp) on seeded random structures -- 3 x 3 blocks (many blocks per chunk, odd block sizes), a BA
// shape of 6- and 3-wide columns with a camera row of several hundred blocks, 1 x 1 blocks (a block per value), a block column
// of width 11, a structure that ends exactly at a chunk boundary, an empty structure -- checked against a plain restatement:
// the offsets are the running sum of the block sizes, and the walk the kernel makes (the fixed number of halvings between two chunk
// entries, then one value forward) lands on the block and the position a linear scan finds for every packed value.
// Built with AddressSanitizer + UBSan on the CPU.  Prints one line per structure ("<name>: blocks .. values .. chunks .. ok")
// and exits 0, or says what is wrong and exits 1.
#include "pattern_outer_tables.h"
#include <cstdio>
#include <random>
using namespace slampp;

#define REQUIRE(cond) do { if(!(cond)) { printf("%s: value %ld: failed: %s (line %d)\n", name, long(e), #cond, __LINE__); return false; } } while(0)

static bool check(const char *name, const std::vector<int64_t> &cs, const std::vector<int64_t> &ptr, const std::vector<int32_t> &brow)
{
	const int64_t n = int64_t(cs.size()) - 1, n_blocks = int64_t(brow.size());
	int64_t e = -1;
	PatternOuterTables T;
	pattern_outer_build_tables(n, cs, ptr, brow, T);
	REQUIRE(int64_t(T.boff.size()) == n_blocks + 1 && int64_t(T.row0.size()) == n_blocks && int64_t(T.col0.size()) == n_blocks &&
		int64_t(T.rows.size()) == n_blocks);
	REQUIRE(T.n_chunks == (T.n_values + pattern_outer_CHUNK - 1) / pattern_outer_CHUNK && int64_t(T.chunk.size()) == T.n_chunks + 1);
	// the linear scan: block, row and column of every packed value
	std::vector<int32_t> blk_of, row_of, col_of;
	for(int64_t c = 0; c < n; ++ c) {
		for(int64_t k = ptr[size_t(c)]; k < ptr[size_t(c) + 1]; ++ k) {
			const int32_t r = brow[size_t(k)];
			REQUIRE(T.boff[size_t(k)] == int64_t(blk_of.size()));
			REQUIRE(T.row0[size_t(k)] == cs[size_t(r)] && T.col0[size_t(k)] == cs[size_t(c)] && T.rows[size_t(k)] == cs[size_t(r) + 1] - cs[size_t(r)]);
			for(int64_t j = cs[size_t(c)]; j < cs[size_t(c) + 1]; ++ j) {
				for(int64_t i = cs[size_t(r)]; i < cs[size_t(r) + 1]; ++ i) {
					blk_of.push_back(int32_t(k));
					row_of.push_back(int32_t(i));
					col_of.push_back(int32_t(j));
				}
			}
		}
	}
	REQUIRE(T.n_values == int64_t(blk_of.size()) && T.boff[size_t(n_blocks)] == T.n_values);
	// the kernel's walk, two values per thread
	for(e = 0; e < T.n_values; e += 2) {
		const int64_t q = e / pattern_outer_CHUNK;
		REQUIRE(q + 1 < int64_t(T.chunk.size()));
		int32_t k = T.chunk[size_t(q)], k_hi = T.chunk[size_t(q) + 1];
		REQUIRE(k >= 0 && k <= k_hi && k_hi < n_blocks);
		for(int n_step = 0; n_step < T.n_bisect_steps; ++ n_step) { // (a fixed number of halvings, as in the kernel)
			const int32_t k_mid = k + (k_hi - k + 1) / 2;
			REQUIRE(k_mid >= k && k_mid <= k_hi);
			if(T.boff[size_t(k_mid)] <= e)
				k = k_mid;
			else
				k_hi = k_mid - 1;
		}
		REQUIRE(k == k_hi);
		REQUIRE(k == blk_of[size_t(e)]);
		const uint32_t dr = uint32_t(T.rows[size_t(k)]), n_local = uint32_t(e - T.boff[size_t(k)]);
		uint32_t j = n_local / dr, i = n_local - j * dr;
		REQUIRE(T.row0[size_t(k)] + int32_t(i) == row_of[size_t(e)] && T.col0[size_t(k)] + int32_t(j) == col_of[size_t(e)]);
		if(e + 1 < T.n_values) {
			if(e + 1 == T.boff[size_t(k) + 1]) {
				REQUIRE(k + 1 < n_blocks);
				++ k;
				i = j = 0;
			} else if(++ i == dr) {
				i = 0;
				++ j;
			}
			REQUIRE(k == blk_of[size_t(e) + 1]);
			REQUIRE(T.row0[size_t(k)] + int32_t(i) == row_of[size_t(e) + 1] && T.col0[size_t(k)] + int32_t(j) == col_of[size_t(e) + 1]);
		}
	}
	e = -1;
	printf("%s: blocks %ld values %ld chunks %ld ok\n", name, long(n_blocks), long(T.n_values), long(T.n_chunks));
	return true;
}

// block columns of the given widths; column c holds its diagonal block and, with probability f_fill, every block above it
// (row 0 always where b_full_first_row: the long camera row)
static bool random_structure(const char *name, const std::vector<int> &dims, double f_fill, bool b_full_first_row, std::mt19937 &rng)
{
	const int64_t n = int64_t(dims.size());
	std::vector<int64_t> cs(size_t(n) + 1, 0), ptr(1, 0);
	std::vector<int32_t> brow;
	std::uniform_real_distribution<double> u(0, 1);
	for(int64_t c = 0; c < n; ++ c) {
		cs[size_t(c) + 1] = cs[size_t(c)] + dims[size_t(c)];
		for(int64_t r = 0; r < c; ++ r) {
			if((r == 0 && b_full_first_row) || u(rng) < f_fill)
				brow.push_back(int32_t(r));
		}
		brow.push_back(int32_t(c));
		ptr.push_back(int64_t(brow.size()));
	}
	return check(name, cs, ptr, brow);
}

int main()
{
	std::mt19937 rng(11);
	bool b_ok = true;
	b_ok = random_structure("blocks3", std::vector<int>(300, 3), 0.02, false, rng) && b_ok;
	{
		std::vector<int> dims(4, 6);
		dims.resize(4 + 700, 3);
		b_ok = random_structure("ba_long_row", dims, 0.0, true, rng) && b_ok;
	}
	b_ok = random_structure("scalars", std::vector<int>(90, 1), 0.3, false, rng) && b_ok;
	{
		std::vector<int> dims(40, 7);
		dims[17] = 11;
		b_ok = random_structure("width11", dims, 0.1, false, rng) && b_ok;
	}
	b_ok = random_structure("one_chunk_exactly", std::vector<int>(2, 8), 0.0, false, rng) && b_ok; // 2 x 64 values
	b_ok = random_structure("one_block", std::vector<int>(1, 5), 0.0, false, rng) && b_ok;
	b_ok = check("empty", std::vector<int64_t>(1, 0), std::vector<int64_t>(1, 0), std::vector<int32_t>()) && b_ok;
	return b_ok? 0 : 1;
}
