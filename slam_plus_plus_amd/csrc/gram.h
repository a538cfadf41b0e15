// gram.h -- the tall-skinny product out = A^T B in a fixed summation order (gram.hip): slampp_hip_gram_device_async
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace slampp {

// gram_MAX_COLUMNS: most columns of either operand (SLAMPP_HIP_GRAM_MAX_COLUMNS); gram_CHUNK_ROWS: rows of a chunk while
// that gives at most gram_MAX_CHUNKS chunks, beyond which a chunk grows (in whole tiles of gram_TILE_ROWS rows) so that the
// number stays at most gram_MAX_CHUNKS
enum { gram_MAX_COLUMNS = 48, gram_TILE_ROWS = 64, gram_CHUNK_ROWS = 2048, gram_MAX_CHUNKS = 256,
	gram_PARTIAL_DOUBLES = gram_MAX_CHUNKS * gram_MAX_COLUMNS * gram_MAX_COLUMNS };

// rows of a chunk and number of chunks for n_rows rows: they depend on n_rows alone
int64_t gram_chunk_rows(int64_t n_rows);
int gram_chunk_num(int64_t n_rows);

// out(i, j) = sum over r < n_rows of a_i[r] b_j[r], a_i = p_a + i * n_lda, b_j = p_b + j * n_ldb, out(i, j) = p_out[i + j * n_ldo];
// 1 <= n_ka, n_kb <= gram_MAX_COLUMNS.  Two launches: a workgroup per chunk of rows sums its n_ka x n_kb partial block (every
// entry in one fixed order of its rows), then a lane per entry adds the partial blocks in chunk order.  p_partials:
// gram_PARTIAL_DOUBLES doubles of workspace.  No atomics; enqueue-only.
void gram_enqueue(const double *p_a, int64_t n_lda, int n_ka, const double *p_b, int64_t n_ldb, int n_kb, int64_t n_rows,
	double *p_partials, double *p_out, int64_t n_ldo, hipStream_t stream);

} // namespace slampp
