// gram.hip -- out = A^T B for two tall-skinny operands of at most 48 columns, in a fixed summation order: the Gram matrix
// Y^T Y of the half-solved columns Y = L^-1 P B^T is B Lambda^-1 B^T (slampp_hip_gram_device_async); slampp_hip_dot_device_async
// grown to a block.
//
// The rows are cut into chunks whose length and number depend on the number of rows alone (gram.h).  A workgroup takes one
// chunk, gram_TILE_ROWS rows at a time: it stages the tile of both operands (of the one, where a and b are the same array)
// in LDS, transposed -- the columns of a row next to each other.  Its 16 waves are four groups of four; a group multiplies
// its quarter of every tile's rows, four rows to a v_mfma_f64_16x16x4, a wave per 16 output columns, and the four groups'
// sums are added in group order.  The partial block of every chunk goes to the workspace; a second launch adds them in chunk
// order, a lane per entry.  So every entry is one fixed sequence of operations whatever runs beside it: two calls give the
// same bits, and with a == b entry (i, j) and entry (j, i) are the same products added in the same order (the instruction sums
// its four rows in one order for every entry).
//
// LDS: a tile row is 49 doubles long.  Staging writes walk down a tile column (lane = row), an odd stride in doubles: the
// lanes of a write group fall on banks of their own.  An operand read takes 16 consecutive doubles of each of four rows.
#include <hip/hip_runtime.h>
#include "gram.h"
#include "solver.h"

namespace slampp {

enum { GRAM_LD = gram_MAX_COLUMNS | 1, GRAM_SIDE = 16, GRAM_PER_LANE = gram_MAX_COLUMNS / GRAM_SIDE };

int64_t gram_chunk_rows(int64_t n_rows)
{
	if(n_rows <= int64_t(gram_CHUNK_ROWS) * gram_MAX_CHUNKS)
		return gram_CHUNK_ROWS;
	const int64_t n_even = (n_rows + gram_MAX_CHUNKS - 1) / gram_MAX_CHUNKS;
	return (n_even + gram_TILE_ROWS - 1) / gram_TILE_ROWS * gram_TILE_ROWS;
}

int gram_chunk_num(int64_t n_rows)
{
	const int64_t n_chunk = gram_chunk_rows(n_rows);
	return int((n_rows + n_chunk - 1) / n_chunk);
}

// A tile of one operand on its way into LDS, in two steps: gram_fetch() loads the lane's share from memory into registers
// (element e = lane + 1024 t is row e % 64 of column e / 64: a wave reads 64 consecutive doubles of one column), gram_store()
// puts it at s[r * GRAM_LD + i].  The fetch of the next tile is issued before the products of the current one, so its trip to
// memory runs beside them.  Rows past the end of the chunk are staged as zeros.
// GRAM_GROUPS groups of four waves share a workgroup and its staged tile: group g multiplies the rows [g, g + 1) *
// GRAM_GROUP_ROWS of every tile into accumulators of its own, and the groups' sums are added in group order at the end.  One
// group alone is one wave per SIMD, with nothing to hide the latency of its LDS reads behind.
enum { GRAM_GROUPS = 4, GRAM_GROUP_LANES = GRAM_SIDE * GRAM_SIDE, GRAM_THREADS = GRAM_GROUPS * GRAM_GROUP_LANES,
	GRAM_FETCH = gram_MAX_COLUMNS * gram_TILE_ROWS / GRAM_THREADS, GRAM_GROUP_ROWS = gram_TILE_ROWS / GRAM_GROUPS };

__device__ __forceinline__ void gram_fetch(double (&regs)[GRAM_FETCH], const double *__restrict__ p, int64_t n_ld, int k, int64_t row0, int n_here)
{
	#pragma unroll
	for(int t = 0; t < GRAM_FETCH; ++ t) {
		const int e = threadIdx.x + GRAM_THREADS * t, i = e / gram_TILE_ROWS, r = e - i * gram_TILE_ROWS;
		regs[t] = (i < k && r < n_here)? p[int64_t(i) * n_ld + row0 + r] : 0.0;
	}
}

__device__ __forceinline__ void gram_store(double *s, const double (&regs)[GRAM_FETCH], int k)
{
	#pragma unroll
	for(int t = 0; t < GRAM_FETCH; ++ t) {
		const int e = threadIdx.x + GRAM_THREADS * t, i = e / gram_TILE_ROWS, r = e - i * gram_TILE_ROWS;
		if(i < k)
			s[r * GRAM_LD + i] = regs[t];
	}
}

// One chunk on the matrix cores: v_mfma_f64_16x16x4 multiplies a 16 x 4 piece of A^T by a 4 x 16 piece of B and adds the
// 16 x 16 result, one operand value of each per lane (lane l: A^T[i = l & 15][row l >> 4], B[row l >> 4][j = l & 15]; result
// register r of lane l: entry (i = (l >> 4) + 4 r, j = l & 15)).  Within a group, wave w owns the 16 output columns 16 w ..
// (a wave past the operands' columns, and always the fourth, only stages) and up to three 16 x 16 blocks down them, and takes
// the group's 16 rows of a tile four at a time, in order: per four rows a lane reads four doubles from LDS.  (The plain
// multiply-add form this replaced -- a lane per 3 x 3 entries, six LDS reads and nine multiply-adds per row -- measured
// 0.198 ms where this measures 0.140 ms at 600 000 rows x 48 columns, and 0.100 against 0.096 ms at 8 columns.)  Rows past
// the end of a chunk are staged as zeros and add nothing; columns past an operand's last are read from its last column and
// their results are not stored.
typedef double gram_v4d __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(GRAM_THREADS)
gram_chunk_kernel(const double *__restrict__ p_a, int64_t n_lda, int n_ka, const double *__restrict__ p_b, int64_t n_ldb, int n_kb,
	int64_t n_rows, int64_t n_chunk_rows, double *__restrict__ p_partials)
{
	__shared__ double s_a[gram_TILE_ROWS * GRAM_LD], s_b[gram_TILE_ROWS * GRAM_LD];
	const bool b_same = p_a == p_b && n_lda == n_ldb && n_ka == n_kb;
	const double *s_bb = b_same? s_a : s_b;
	const int n_group = threadIdx.x / GRAM_GROUP_LANES, n_lane = threadIdx.x % GRAM_GROUP_LANES;
	const int w = n_lane >> 6, l = n_lane & 63, lc = l & 15, lr = l >> 4;
	const int nu = (n_ka + GRAM_SIDE - 1) / GRAM_SIDE, nv = (n_kb + GRAM_SIDE - 1) / GRAM_SIDE;
	const bool b_owner = w < nv;
	const int jb = (GRAM_SIDE * w + lc < n_kb)? GRAM_SIDE * w + lc : n_kb - 1;
	int ia[GRAM_PER_LANE];
	#pragma unroll
	for(int u = 0; u < GRAM_PER_LANE; ++ u)
		ia[u] = (GRAM_SIDE * u + lc < n_ka)? GRAM_SIDE * u + lc : n_ka - 1;
	gram_v4d acc[GRAM_PER_LANE];
	#pragma unroll
	for(int u = 0; u < GRAM_PER_LANE; ++ u)
		acc[u] = gram_v4d{0.0, 0.0, 0.0, 0.0};
	const int64_t row_begin = int64_t(blockIdx.x) * n_chunk_rows;
	const int64_t row_end = (row_begin + n_chunk_rows < n_rows)? row_begin + n_chunk_rows : n_rows;
	double fa[GRAM_FETCH], fb[GRAM_FETCH];
	{
		const int n_first = int((row_end - row_begin < gram_TILE_ROWS)? row_end - row_begin : int64_t(gram_TILE_ROWS));
		gram_fetch(fa, p_a, n_lda, n_ka, row_begin, n_first);
		if(!b_same)
			gram_fetch(fb, p_b, n_ldb, n_kb, row_begin, n_first);
	}
	for(int64_t row0 = row_begin; row0 < row_end; row0 += gram_TILE_ROWS) {
		__syncthreads(); // (the tile before this one has been read)
		gram_store(s_a, fa, n_ka);
		if(!b_same)
			gram_store(s_b, fb, n_kb);
		__syncthreads();
		const int64_t row_next = row0 + gram_TILE_ROWS;
		if(row_next < row_end) {
			const int n_next = int((row_end - row_next < gram_TILE_ROWS)? row_end - row_next : int64_t(gram_TILE_ROWS));
			gram_fetch(fa, p_a, n_lda, n_ka, row_next, n_next);
			if(!b_same)
				gram_fetch(fb, p_b, n_ldb, n_kb, row_next, n_next);
		}
		if(b_owner) { // (wave-uniform)
			const double *p_sa = s_a + (n_group * GRAM_GROUP_ROWS + lr) * GRAM_LD, *p_sb = s_bb + (n_group * GRAM_GROUP_ROWS + lr) * GRAM_LD + jb;
			#pragma unroll
			for(int q = 0; q < GRAM_GROUP_ROWS / 4; ++ q) {
				const double bv = p_sb[4 * q * GRAM_LD];
				const double a0 = p_sa[4 * q * GRAM_LD + ia[0]], a1 = p_sa[4 * q * GRAM_LD + ia[1]], a2 = p_sa[4 * q * GRAM_LD + ia[2]];
				acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, bv, acc[0], 0, 0, 0);
				if(nu > 1)
					acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, bv, acc[1], 0, 0, 0);
				if(nu > 2)
					acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, bv, acc[2], 0, 0, 0);
			}
		}
	}
	// the groups' sums into group 0's, in group order (s_a is free: every tile has been read)
	for(int g = 1; g < GRAM_GROUPS; ++ g) {
		__syncthreads();
		if(n_group == g) {
			#pragma unroll
			for(int u = 0; u < GRAM_PER_LANE; ++ u) {
				#pragma unroll
				for(int r = 0; r < 4; ++ r)
					s_a[(u * 4 + r) * GRAM_GROUP_LANES + n_lane] = acc[u][r];
			}
		}
		__syncthreads();
		if(n_group == 0) {
			#pragma unroll
			for(int u = 0; u < GRAM_PER_LANE; ++ u) {
				#pragma unroll
				for(int r = 0; r < 4; ++ r)
					acc[u][r] += s_a[(u * 4 + r) * GRAM_GROUP_LANES + n_lane];
			}
		}
	}
	if(n_group || !b_owner)
		return;
	double *p_block = p_partials + int64_t(blockIdx.x) * n_ka * n_kb;
	#pragma unroll
	for(int u = 0; u < GRAM_PER_LANE; ++ u) {
		#pragma unroll
		for(int r = 0; r < 4; ++ r) {
			const int i = GRAM_SIDE * u + lr + 4 * r, j = GRAM_SIDE * w + lc;
			if(i < n_ka && j < n_kb)
				p_block[i + j * n_ka] = acc[u][r];
		}
	}
}

// the partial blocks added in chunk order: a lane per entry
__global__ void __launch_bounds__(256)
gram_sum_kernel(const double *__restrict__ p_partials, int n_chunks, int n_ka, int n_kb, double *__restrict__ p_out, int64_t n_ldo)
{
	const int e = blockIdx.x * blockDim.x + threadIdx.x;
	if(e >= n_ka * n_kb)
		return;
	double sum = 0;
	for(int q = 0; q < n_chunks; ++ q)
		sum += p_partials[int64_t(q) * n_ka * n_kb + e];
	const int j = e / n_ka, i = e - j * n_ka;
	p_out[i + j * n_ldo] = sum;
}

void gram_enqueue(const double *p_a, int64_t n_lda, int n_ka, const double *p_b, int64_t n_ldb, int n_kb, int64_t n_rows,
	double *p_partials, double *p_out, int64_t n_ldo, hipStream_t stream)
{
	const int n_chunks = gram_chunk_num(n_rows);
	if(n_chunks > 0) {
		const int64_t n_chunk_rows = gram_chunk_rows(n_rows);
		hipLaunchKernelGGL(gram_chunk_kernel, dim3(unsigned(n_chunks)), dim3(GRAM_THREADS), 0, stream, p_a, n_lda, n_ka, p_b,
			n_ldb, n_kb, n_rows, n_chunk_rows, p_partials);
	}
	hipLaunchKernelGGL(gram_sum_kernel, dim3(unsigned((n_ka * n_kb + 255) / 256)), dim3(256), 0, stream, p_partials, n_chunks, n_ka,
		n_kb, p_out, n_ldo);
	SLAMPP_HIP_CHECK(hipGetLastError());
}

} // namespace slampp
