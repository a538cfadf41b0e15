// pattern_outer_tables.cpp -- the host lookup tables of the outer product on Lambda's pattern (pattern_outer_tables.h)
#include "pattern_outer_tables.h"

#include <stdexcept>

namespace slampp {

void pattern_outer_build_tables(int64_t n, const std::vector<int64_t> &cs, const std::vector<int64_t> &ptr,
	const std::vector<int32_t> &brow, PatternOuterTables &T)
{
	const int64_t n_blocks = (n > 0)? ptr[size_t(n)] : 0;
	if(n_blocks > INT32_MAX || (n > 0 && cs[size_t(n)] > INT32_MAX))
		throw std::domain_error("pattern_outer: more than 2^31 - 1 blocks or scalars");
	T.boff.assign(size_t(n_blocks) + 1, 0);
	T.row0.assign(size_t(n_blocks), 0);
	T.col0.assign(size_t(n_blocks), 0);
	T.rows.assign(size_t(n_blocks), 0);
	int64_t n_off = 0;
	for(int64_t c = 0; c < n; ++ c) {
		const int64_t w = cs[size_t(c) + 1] - cs[size_t(c)];
		for(int64_t k = ptr[size_t(c)]; k < ptr[size_t(c) + 1]; ++ k) {
			const int32_t r = brow[size_t(k)];
			const int64_t h = cs[size_t(r) + 1] - cs[size_t(r)];
			T.boff[size_t(k)] = n_off;
			T.row0[size_t(k)] = int32_t(cs[size_t(r)]);
			T.col0[size_t(k)] = int32_t(cs[size_t(c)]);
			T.rows[size_t(k)] = int32_t(h);
			if(h * w > INT32_MAX)
				throw std::domain_error("pattern_outer: a block of more than 2^31 - 1 values");
			n_off += h * w;
		}
	}
	T.boff[size_t(n_blocks)] = n_off;
	T.n_values = n_off;
	T.n_chunks = (n_off + pattern_outer_CHUNK - 1) / pattern_outer_CHUNK;
	T.chunk.assign(size_t(T.n_chunks) + 1, int32_t(n_blocks > 0? n_blocks - 1 : 0));
	int64_t k = 0;
	for(int64_t q = 0; q < T.n_chunks; ++ q) { // (the blocks are not empty: boff ascends strictly)
		const int64_t e = q * pattern_outer_CHUNK;
		while(T.boff[size_t(k) + 1] <= e)
			++ k;
		T.chunk[size_t(q)] = int32_t(k);
	}
	T.n_bisect_steps = 0;
	for(int64_t q = 0; q < T.n_chunks; ++ q) {
		while((int64_t(1) << T.n_bisect_steps) < int64_t(T.chunk[size_t(q) + 1]) - T.chunk[size_t(q)] + 1)
			++ T.n_bisect_steps;
	}
}

} // namespace slampp
