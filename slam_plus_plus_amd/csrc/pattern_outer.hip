// pattern_outer.hip -- out = alpha P(a, b) + beta out on Lambda's block pattern, where P(a, b) is the adjoint of the product
// y = Lambda x with respect to the packed values (<v, P(a, b)> = a^T M(v) b for the symmetric M(v) of multiply.hip):
//   out(r, c) = alpha (a_r b_c^T + b_r a_c^T) + beta out(r, c)   for a stored block r < c,
//   out(r, r) = alpha  a_r b_r^T              + beta out(r, r)   for a diagonal block (the full d x d block).
// A pure stream over the packed array: with beta = 0 it writes 8 n_values bytes and reads the two vectors, which stay in the
// caches.  So the work is cut by packed VALUES, not by blocks: a thread owns pairs of consecutive values and writes each with one
// 16-byte store -- a wave instruction stores 1 KiB contiguous --, whatever the block sizes are (a wave per block would leave
// 9-, 18-, 36- and 49-value blocks mostly idle).  A thread finds the block of a pair's first value by bisection between the
// first block of its chunk of pattern_outer_CHUNK values and the first block of the next chunk (a host table, built at the
// first call after a set_structure); the second value is the next one of that block or the first one of the block behind it
// (3 x 3 and 7 x 7 blocks have odd sizes: the pairs straddle blocks).  A member whose out is not 16-byte aligned is written with
// 8-byte stores, with the same values.  No atomics, no reductions: every value is at most two products and one add, in one
// fixed form (explicit fused multiply-adds), so two calls -- batched or not, aligned or not -- give the same bits.
// The sum over several vector pairs (slampp_hip_pattern_outer_sum) is the same kernel with a loop over the terms.
#include "pattern_outer.h"
#include "pattern_outer_tables.h"
#include "solver.h"

namespace slampp {

struct TOuterTables {
	const int64_t *boff;   // [n_blocks + 1]
	const int32_t *row0;   // [n_blocks]
	const int32_t *col0;   // [n_blocks]
	const int32_t *rows;   // [n_blocks]
	const int32_t *chunk;  // [n_chunks + 1]
	int64_t n_values;
	int n_bisect_steps;    // halvings that find a block between two chunk entries
};

struct CPatternOuterState {
	CDevArray<int64_t> d_boff;
	CDevArray<int32_t> d_row0, d_col0, d_rows, d_chunk;
	TOuterTables t;
};

// the value at scalar row n_r of block row r and scalar row n_c of block column c, before beta (no branch: the loads of a
// diagonal block's second product are made and dropped)
__device__ __forceinline__ double outer_value(const double *__restrict__ a, const double *__restrict__ b, int32_t n_r, int32_t n_c,
	bool b_diag, double f_alpha)
{
	const double f = a[n_r] * b[n_c], f_both = __fma_rn(b[n_r], a[n_c], f);
	return f_alpha * (b_diag? f : f_both);
}

// A workgroup takes a tile of outer_PAIRS x 512 values, a thread pair u = 0 .. outer_PAIRS - 1 of it at 512 u + 2 threadIdx.x:
// every wave instruction still stores 1 KiB contiguous, and a thread has outer_PAIRS independent chains of dependent loads
// (chunk entry -> n_bisect_steps block offsets -> the block's record -> the vectors) in flight, whose latency is what
// bounds this kernel.  Each phase runs over all pairs before the next one begins, and none of them branches, so that the
// loads of a phase are issued together.
enum { outer_PAIRS = 4 };

// B_SUM (slampp_hip_pattern_outer_sum): one member, out = alpha sum over the n_terms vector pairs p_a + k n_a_stride,
// p_b + k n_b_stride + beta out: the thread keeps its values in registers over the terms, added in ascending k, and writes
// out once; the first term is computed as the plain kernel computes it, so one term gives that kernel's bits
template <bool B_SUM>
__global__ void __launch_bounds__(256)
pattern_outer_kernel(TOuterTables t, const double *__restrict__ p_a, int64_t n_a_stride, const double *__restrict__ p_b,
	int64_t n_b_stride, double *p_out, int64_t n_out_stride, double f_alpha, double f_beta, int n_terms)
{
	const double *__restrict__ a = p_a + (B_SUM? 0 : int64_t(blockIdx.y) * n_a_stride);
	const double *__restrict__ b = p_b + (B_SUM? 0 : int64_t(blockIdx.y) * n_b_stride);
	double *out = p_out + (B_SUM? 0 : int64_t(blockIdx.y) * n_out_stride);
	const int64_t n_first = int64_t(blockIdx.x) * (512 * outer_PAIRS) + 2 * threadIdx.x;
	int64_t e[outer_PAIRS];
	int32_t k[outer_PAIRS], k_hi[outer_PAIRS];
	bool b_mine[outer_PAIRS];
	#pragma unroll
	for(int u = 0; u < outer_PAIRS; ++ u) {
		e[u] = n_first + 512 * u;
		b_mine[u] = e[u] < t.n_values;
		if(!b_mine[u])
			e[u] = 0; // (computed like any other pair, not stored)
		const int64_t q = e[u] / pattern_outer_CHUNK;
		k[u] = t.chunk[q];
		k_hi[u] = t.chunk[q + 1];
	}
	// the block of value e: the last one that begins at or before it, between the first block of its chunk and the first one of
	// the next chunk (k <= k_mid <= k_hi in every step; once k == k_hi the steps change nothing)
	for(int n_step = 0; n_step < t.n_bisect_steps; ++ n_step) {
		#pragma unroll
		for(int u = 0; u < outer_PAIRS; ++ u) {
			const int32_t k_mid = k[u] + (k_hi[u] - k[u] + 1) / 2;
			const bool b_upper = t.boff[k_mid] <= e[u];
			k[u] = (b_upper)? k_mid : k[u];
			k_hi[u] = (b_upper)? k_hi[u] : k_mid - 1;
		}
	}
	// the second value of a pair is the next one of the same block, or the first one of the block behind it (the blocks are not empty)
	int32_t n_r0[outer_PAIRS], n_c0[outer_PAIRS], n_r1[outer_PAIRS], n_c1[outer_PAIRS];
	bool b_diag0[outer_PAIRS], b_diag1[outer_PAIRS], b_second[outer_PAIRS];
	#pragma unroll
	for(int u = 0; u < outer_PAIRS; ++ u) {
		b_second[u] = e[u] + 1 < t.n_values;
		const bool b_next = b_second[u] && e[u] + 1 == t.boff[k[u] + 1];
		const int32_t k1 = (b_next)? k[u] + 1 : k[u];
		const int32_t r0 = t.row0[k[u]], c0 = t.col0[k[u]], r1 = t.row0[k1], c1 = t.col0[k1];
		const uint32_t dr = uint32_t(t.rows[k[u]]), n_local = uint32_t(e[u] - t.boff[k[u]]);
		const uint32_t j = n_local / dr, i = n_local - j * dr;
		const bool b_wrap = i + 1 == dr;
		const uint32_t i1 = (b_next || b_wrap)? 0 : i + 1, j1 = (b_next)? 0 : (b_wrap)? j + 1 : j;
		n_r0[u] = r0 + int32_t(i);
		n_c0[u] = c0 + int32_t(j);
		b_diag0[u] = r0 == c0;
		n_r1[u] = (b_second[u])? r1 + int32_t(i1) : n_r0[u];
		n_c1[u] = (b_second[u])? c1 + int32_t(j1) : n_c0[u];
		b_diag1[u] = r1 == c1;
	}
	double f0[outer_PAIRS], f1[outer_PAIRS];
	#pragma unroll
	for(int u = 0; u < outer_PAIRS; ++ u) {
		if(!B_SUM) {
			f0[u] = outer_value(a, b, n_r0[u], n_c0[u], b_diag0[u], f_alpha);
			f1[u] = outer_value(a, b, n_r1[u], n_c1[u], b_diag1[u], f_alpha);
		} else {
			f0[u] = outer_value(a, b, n_r0[u], n_c0[u], b_diag0[u], 1.0);
			f1[u] = outer_value(a, b, n_r1[u], n_c1[u], b_diag1[u], 1.0);
		}
	}
	if(B_SUM) {
		for(int k = 1; k < n_terms; ++ k) {
			const double *__restrict__ a_k = a + int64_t(k) * n_a_stride, *__restrict__ b_k = b + int64_t(k) * n_b_stride;
			#pragma unroll
			for(int u = 0; u < outer_PAIRS; ++ u) {
				f0[u] += outer_value(a_k, b_k, n_r0[u], n_c0[u], b_diag0[u], 1.0);
				f1[u] += outer_value(a_k, b_k, n_r1[u], n_c1[u], b_diag1[u], 1.0);
			}
		}
		#pragma unroll
		for(int u = 0; u < outer_PAIRS; ++ u) {
			f0[u] *= f_alpha;
			f1[u] *= f_alpha;
		}
	}
	const bool b_aligned = (reinterpret_cast<uintptr_t>(out) & 15) == 0; // (the same for the whole member: no divergence)
	#pragma unroll
	for(int u = 0; u < outer_PAIRS; ++ u) {
		if(!b_mine[u])
			continue;
		if(b_second[u] && b_aligned) {
			double2 *p_pair = reinterpret_cast<double2*>(out + e[u]);
			if(f_beta != 0) {
				const double2 v_old = *p_pair;
				f0[u] = __fma_rn(f_beta, v_old.x, f0[u]);
				f1[u] = __fma_rn(f_beta, v_old.y, f1[u]);
			}
			*p_pair = make_double2(f0[u], f1[u]);
		} else {
			out[e[u]] = (f_beta != 0)? __fma_rn(f_beta, out[e[u]], f0[u]) : f0[u];
			if(b_second[u])
				out[e[u] + 1] = (f_beta != 0)? __fma_rn(f_beta, out[e[u] + 1], f1[u]) : f1[u];
		}
	}
}

CPatternOuterState *pattern_outer_setup(int64_t n, const std::vector<int64_t> &cs, const std::vector<int64_t> &ptr,
	const std::vector<int32_t> &brow, hipStream_t stream)
{
	PatternOuterTables T;
	pattern_outer_build_tables(n, cs, ptr, brow, T);
	if((T.n_values + 512 * outer_PAIRS - 1) / (512 * outer_PAIRS) > INT32_MAX)
		throw std::domain_error("pattern_outer: too many values for one launch");
	CPatternOuterState *p = new CPatternOuterState();
	try {
		CPatternOuterState &S = *p;
		S.d_boff.Upload(T.boff, stream);
		S.d_row0.Upload(T.row0, stream);
		S.d_col0.Upload(T.col0, stream);
		S.d_rows.Upload(T.rows, stream);
		S.d_chunk.Upload(T.chunk, stream);
		SLAMPP_HIP_CHECK(hipStreamSynchronize(stream)); // the host vectors live on this stack frame
		const TOuterTables t = {S.d_boff.p(), S.d_row0.p(), S.d_col0.p(), S.d_rows.p(), S.d_chunk.p(), T.n_values, T.n_bisect_steps};
		S.t = t;
	} catch(...) {
		delete p;
		throw;
	}
	return p;
}

void pattern_outer_destroy(CPatternOuterState *p) { delete p; }

size_t pattern_outer_device_bytes(const CPatternOuterState *p)
{
	return p? p->d_boff.n_Bytes() + p->d_row0.n_Bytes() + p->d_col0.n_Bytes() + p->d_rows.n_Bytes() + p->d_chunk.n_Bytes() : 0;
}

void pattern_outer_enqueue(const CPatternOuterState &S, int n_batch, const double *p_a, int64_t n_a_stride, const double *p_b,
	int64_t n_b_stride, double *p_out, int64_t n_out_stride, double f_alpha, double f_beta, hipStream_t st)
{
	if(!S.t.n_values)
		return;
	hipLaunchKernelGGL(pattern_outer_kernel<false>, dim3(unsigned((S.t.n_values + 512 * outer_PAIRS - 1) / (512 * outer_PAIRS)), unsigned(n_batch)), dim3(256), 0, st, S.t,
		p_a, n_a_stride, p_b, n_b_stride, p_out, n_out_stride, f_alpha, f_beta, 1);
	SLAMPP_HIP_CHECK(hipGetLastError());
}

void pattern_outer_sum_enqueue(const CPatternOuterState &S, int n_terms, const double *p_a, int64_t n_a_stride, const double *p_b,
	int64_t n_b_stride, double *p_out, double f_alpha, double f_beta, hipStream_t st)
{
	if(!S.t.n_values)
		return;
	hipLaunchKernelGGL(pattern_outer_kernel<true>, dim3(unsigned((S.t.n_values + 512 * outer_PAIRS - 1) / (512 * outer_PAIRS))), dim3(256), 0, st, S.t,
		p_a, n_a_stride, p_b, n_b_stride, p_out, 0, f_alpha, f_beta, n_terms);
	SLAMPP_HIP_CHECK(hipGetLastError());
}

} // namespace slampp

// the tables of the current structure, built at the first outer product after a set_structure (the lifetime of the
// product's row lists: Require_Multiply)
void slampp_hip_solver::Require_Pattern_Outer()
{
	if(p_outer && b_outer_valid)
		return;
	if(p_outer) {
		SLAMPP_HIP_CHECK(hipStreamSynchronize(stream)); // (a call enqueued earlier may still read the old tables)
		slampp::pattern_outer_destroy(p_outer);
		p_outer = 0;
	}
	p_outer = slampp::pattern_outer_setup(int64_t(cumsum.size()) - 1, cumsum, bcol_ptr, brow, stream);
	b_outer_valid = true;
}
