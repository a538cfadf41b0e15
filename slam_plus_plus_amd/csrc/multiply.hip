// multiply.hip -- y = alpha Lambda x + beta y for the symmetric Lambda whose upper blocks are stored (block-CSC, as the
// caller gave it to slampp_hip_set_structure), without atomics and in a fixed order of sums: a gather per block row.
//
// Block row i of the full symmetric matrix is
//   - the blocks (r, i), r <= i, of block column i, transposed (the diagonal block as it is stored: a full d x d block),
//   - the stored blocks (i, c), c > i: the row list, built on the host (block offset and column of every such block, by
//     ascending c),
// taken in that order, which is ascending block column of the full matrix.  Two regimes by the number of blocks in a row:
//   short rows (pose graphs, landmark rows: a handful of blocks)   multiply_short_kernel: eight lanes per block row, 32 rows
//       per workgroup; lane l takes the row's entries l, l + 8, ...; the eight partial sums meet in a butterfly;
//   long rows (a BA camera row: thousands of 6 x 3 blocks)          cut into chunks of multiply_CHUNK entries, a wave each
//       (multiply_long_kernel: lane l takes the chunk's entries l, l + 64, ...), partial results to a workspace, summed in chunk
//       order by multiply_long_finish_kernel.
// A row is long when it has more than multiply_LONG_ROW entries.  Block dimensions up to 8 run unrolled over the largest
// dimension of the structure; a structure with a wider block column goes through multiply_generic_kernel (a wave per block
// row, a lane per scalar row, every sum sequential: slow and correct).  The fixed-order reductions of the dot product and
// the infinity norm are here too.
#include "multiply.h"
#include "solver.h"

#include <algorithm>
#include <stdexcept>

namespace slampp {

struct TMulTables {
	const int64_t *cs;     // [n + 1] scalar offset of every block column
	const int64_t *ptr;    // [n + 1] block column pointers
	const int32_t *brow;   // [n_blocks]
	const int64_t *boff;   // [n_blocks] offset of every stored block in the packed values
	const int64_t *rptr;   // [n + 1] row lists: the blocks (i, c), c > i
	const int64_t *roff;   // [n_offdiag] their offsets in the packed values
	const int32_t *rcol;   // [n_offdiag] their block columns
	int64_t n;
	int64_t n_long;        // rows with more entries than this belong to the chunked kernels
};

struct CMultiplyState {
	CDevArray<int64_t> d_cs, d_ptr, d_boff, d_rptr, d_roff, d_chunks, d_long_rows;
	CDevArray<int32_t> d_brow, d_rcol;
	CDevArray<double> d_partial; // [n_chunks * 8]
	TMulTables t;
	int64_t n_chunks, n_long_rows;
	int n_max_dim, n_long_row;
};

// entry e of block row i (n_col = blocks of its own column): where the block is, which block column of x it multiplies
// and whether it is read transposed
__device__ __forceinline__ void mul_entry(const TMulTables &t, int64_t i, int64_t n_col, int64_t e, int64_t &r_off, int64_t &r_other,
	bool &r_b_trans)
{
	if(e < n_col) {
		const int64_t k = t.ptr[i] + e;
		r_other = t.brow[k];
		r_off = t.boff[k];
		r_b_trans = r_other != i;
	} else {
		const int64_t j = t.rptr[i] + (e - n_col);
		r_other = t.rcol[j];
		r_off = t.roff[j];
		r_b_trans = false;
	}
}

// acc += B x_o (B: di x dn) or B^T x_o (B: dn x di), column-major, unrolled over D >= di, dn
template <int D>
__device__ __forceinline__ void mul_block(double (&acc)[D], const double *__restrict__ B, const double *__restrict__ xo, int di, int dn,
	bool b_trans)
{
	#pragma unroll
	for(int b = 0; b < D; ++ b) {
		if(b < dn) {
			const double xb = xo[b];
			#pragma unroll
			for(int a = 0; a < D; ++ a) {
				if(a < di)
					acc[a] += (b_trans? B[b + a * dn] : B[a + b * di]) * xb;
			}
		}
	}
}

template <int D>
__global__ void __launch_bounds__(256)
multiply_short_kernel(TMulTables t, const double *__restrict__ A, const double *__restrict__ x, double *y, double f_alpha, double f_beta)
{
	enum { LANES = 8 };
	const int64_t i = (int64_t(blockIdx.x) * 256 + threadIdx.x) / LANES;
	const int sub = threadIdx.x % LANES;
	int64_t n_col = 0, n_ent = 0, y0 = 0;
	int di = 0;
	if(i < t.n) {
		n_col = t.ptr[i + 1] - t.ptr[i];
		n_ent = n_col + (t.rptr[i + 1] - t.rptr[i]);
		y0 = t.cs[i];
		di = int(t.cs[i + 1] - y0);
	}
	const bool b_mine = i < t.n && n_ent <= t.n_long;
	double acc[D];
	#pragma unroll
	for(int a = 0; a < D; ++ a)
		acc[a] = 0;
	if(b_mine) {
		for(int64_t e = sub; e < n_ent; e += LANES) {
			int64_t off, o;
			bool b_trans;
			mul_entry(t, i, n_col, e, off, o, b_trans);
			const int64_t x0 = t.cs[o];
			mul_block<D>(acc, A + off, x + x0, di, int(t.cs[o + 1] - x0), b_trans);
		}
	}
	#pragma unroll
	for(int a = 0; a < D; ++ a) {
		#pragma unroll
		for(int m = 1; m < LANES; m <<= 1)
			acc[a] += __shfl_xor(acc[a], m);
	}
	if(b_mine && sub == 0) {
		#pragma unroll
		for(int a = 0; a < D; ++ a) {
			if(a < di)
				y[y0 + a] = (f_beta != 0)? f_alpha * acc[a] + f_beta * y[y0 + a] : f_alpha * acc[a];
		}
	}
}

// one wave per chunk (row, first entry, one past the last entry); partial results, 8 doubles per chunk
template <int D>
__global__ void __launch_bounds__(64)
multiply_long_kernel(TMulTables t, const int64_t *__restrict__ chunks, const double *__restrict__ A, const double *__restrict__ x,
	double *partial)
{
	const int64_t q = blockIdx.x;
	const int lane = threadIdx.x;
	const int64_t i = chunks[3 * q], e1 = chunks[3 * q + 2];
	const int64_t n_col = t.ptr[i + 1] - t.ptr[i];
	const int di = int(t.cs[i + 1] - t.cs[i]);
	double acc[D];
	#pragma unroll
	for(int a = 0; a < D; ++ a)
		acc[a] = 0;
	for(int64_t e = chunks[3 * q + 1] + lane; e < e1; e += 64) {
		int64_t off, o;
		bool b_trans;
		mul_entry(t, i, n_col, e, off, o, b_trans);
		const int64_t x0 = t.cs[o];
		mul_block<D>(acc, A + off, x + x0, di, int(t.cs[o + 1] - x0), b_trans);
	}
	#pragma unroll
	for(int a = 0; a < D; ++ a) {
		#pragma unroll
		for(int m = 1; m < 64; m <<= 1)
			acc[a] += __shfl_xor(acc[a], m);
	}
	if(lane == 0) {
		#pragma unroll
		for(int a = 0; a < D; ++ a)
			partial[q * 8 + a] = acc[a];
	}
}

// one thread per scalar row of the long block rows (row, first chunk, chunks): the partial results in chunk order
__global__ void __launch_bounds__(64)
multiply_long_finish_kernel(TMulTables t, const int64_t *__restrict__ long_rows, int64_t n_long_rows, const double *__restrict__ partial,
	double *y, double f_alpha, double f_beta)
{
	const int64_t g = int64_t(blockIdx.x) * 64 + threadIdx.x, r = g / 8;
	const int a = int(g % 8);
	if(r >= n_long_rows)
		return;
	const int64_t i = long_rows[3 * r], q0 = long_rows[3 * r + 1], n_q = long_rows[3 * r + 2];
	const int64_t y0 = t.cs[i];
	if(a >= int(t.cs[i + 1] - y0))
		return;
	double sum = 0;
	for(int64_t q = q0; q < q0 + n_q; ++ q)
		sum += partial[q * 8 + a];
	y[y0 + a] = (f_beta != 0)? f_alpha * sum + f_beta * y[y0 + a] : f_alpha * sum;
}

// any block dimension: a wave per block row, lane a computes scalar rows a, a + 64, ... of it, entry by entry
__global__ void __launch_bounds__(64)
multiply_generic_kernel(TMulTables t, const double *__restrict__ A, const double *__restrict__ x, double *y, double f_alpha, double f_beta)
{
	const int64_t i = blockIdx.x;
	const int64_t n_col = t.ptr[i + 1] - t.ptr[i], n_ent = n_col + (t.rptr[i + 1] - t.rptr[i]);
	const int64_t y0 = t.cs[i];
	const int di = int(t.cs[i + 1] - y0);
	for(int a = threadIdx.x; a < di; a += 64) {
		double sum = 0;
		for(int64_t e = 0; e < n_ent; ++ e) {
			int64_t off, o;
			bool b_trans;
			mul_entry(t, i, n_col, e, off, o, b_trans);
			const int64_t x0 = t.cs[o];
			const int dn = int(t.cs[o + 1] - x0);
			const double *B = A + off;
			for(int b = 0; b < dn; ++ b)
				sum += (b_trans? B[b + int64_t(a) * dn] : B[a + int64_t(b) * di]) * x[x0 + b];
		}
		y[y0 + a] = (f_beta != 0)? f_alpha * sum + f_beta * y[y0 + a] : f_alpha * sum;
	}
}

CMultiplyState *multiply_setup(int64_t n, const std::vector<int64_t> &cs, const std::vector<int64_t> &ptr,
	const std::vector<int32_t> &brow, int n_long_row, hipStream_t stream)
{
	const int64_t n_blocks = ptr[size_t(n)];
	std::vector<int64_t> boff(size_t(std::max<int64_t>(n_blocks, 1))), rptr(size_t(n) + 1, 0);
	int64_t n_off = 0, n_max_dim = 0;
	for(int64_t c = 0; c < n; ++ c) {
		const int64_t w = cs[size_t(c) + 1] - cs[size_t(c)];
		n_max_dim = std::max(n_max_dim, w);
		for(int64_t k = ptr[size_t(c)]; k < ptr[size_t(c) + 1]; ++ k) {
			const int32_t r = brow[size_t(k)];
			boff[size_t(k)] = n_off;
			n_off += (cs[size_t(r) + 1] - cs[size_t(r)]) * w;
			if(r < c)
				++ rptr[size_t(r) + 1];
		}
	}
	for(int64_t i = 0; i < n; ++ i)
		rptr[size_t(i) + 1] += rptr[size_t(i)];
	const int64_t n_offdiag = rptr[size_t(n)];
	std::vector<int64_t> roff(size_t(std::max<int64_t>(n_offdiag, 1)));
	std::vector<int32_t> rcol(size_t(std::max<int64_t>(n_offdiag, 1)));
	{
		std::vector<int64_t> fill(rptr.begin(), rptr.end() - 1);
		for(int64_t c = 0; c < n; ++ c) { // (ascending c: every row list comes out sorted by column)
			for(int64_t k = ptr[size_t(c)]; k < ptr[size_t(c) + 1]; ++ k) {
				const int32_t r = brow[size_t(k)];
				if(r < c) {
					const int64_t j = fill[size_t(r)] ++;
					roff[size_t(j)] = boff[size_t(k)];
					rcol[size_t(j)] = int32_t(c);
				}
			}
		}
	}
	// the long rows' chunks (only where the unrolled kernels run: the generic one takes whole rows of any length)
	const int64_t n_long = std::max(n_long_row, 1), n_chunk_len = std::min<int64_t>(multiply_CHUNK, n_long);
	std::vector<int64_t> chunks, long_rows;
	if(n_max_dim <= multiply_MAX_UNROLLED_DIM) {
		for(int64_t i = 0; i < n; ++ i) {
			const int64_t n_ent = (ptr[size_t(i) + 1] - ptr[size_t(i)]) + (rptr[size_t(i) + 1] - rptr[size_t(i)]);
			if(n_ent <= n_long)
				continue;
			const int64_t q0 = int64_t(chunks.size() / 3);
			for(int64_t e = 0; e < n_ent; e += n_chunk_len) {
				chunks.push_back(i);
				chunks.push_back(e);
				chunks.push_back(std::min(e + n_chunk_len, n_ent));
			}
			long_rows.push_back(i);
			long_rows.push_back(q0);
			long_rows.push_back(int64_t(chunks.size() / 3) - q0);
		}
	}
	if(chunks.size() / 3 > size_t(INT32_MAX) || n > INT32_MAX)
		throw std::domain_error("multiply: too many block rows or chunks for one launch");
	CMultiplyState *p = new CMultiplyState();
	try {
		CMultiplyState &M = *p;
		M.n_max_dim = int(n_max_dim);
		M.n_long_row = int(n_long);
		M.n_chunks = int64_t(chunks.size() / 3);
		M.n_long_rows = int64_t(long_rows.size() / 3);
		M.d_cs.Upload(cs, stream);
		M.d_ptr.Upload(ptr, stream);
		M.d_brow.Upload(brow, stream);
		M.d_boff.Upload(boff, stream);
		M.d_rptr.Upload(rptr, stream);
		M.d_roff.Upload(roff, stream);
		M.d_rcol.Upload(rcol, stream);
		M.d_chunks.Upload(chunks, stream);
		M.d_long_rows.Upload(long_rows, stream);
		M.d_partial.Alloc(size_t(std::max<int64_t>(M.n_chunks, 1)) * 8);
		SLAMPP_HIP_CHECK(hipStreamSynchronize(stream)); // the host vectors live on this stack frame
		const TMulTables t = {M.d_cs.p(), M.d_ptr.p(), M.d_brow.p(), M.d_boff.p(), M.d_rptr.p(), M.d_roff.p(), M.d_rcol.p(), n, n_long};
		M.t = t;
	} catch(...) {
		delete p;
		throw;
	}
	return p;
}

void multiply_destroy(CMultiplyState *p) { delete p; }

size_t multiply_device_bytes(const CMultiplyState *p)
{
	return p? p->d_cs.n_Bytes() + p->d_ptr.n_Bytes() + p->d_brow.n_Bytes() + p->d_boff.n_Bytes() + p->d_rptr.n_Bytes() +
		p->d_roff.n_Bytes() + p->d_rcol.n_Bytes() + p->d_chunks.n_Bytes() + p->d_long_rows.n_Bytes() + p->d_partial.n_Bytes() : 0;
}

int multiply_long_row_threshold(const CMultiplyState *p) { return p->n_long_row; }

template <int D>
static void multiply_launch(const CMultiplyState &M, const double *A, const double *x, double *y, double f_alpha, double f_beta,
	hipStream_t st)
{
	hipLaunchKernelGGL((multiply_short_kernel<D>), dim3(unsigned((M.t.n * 8 + 255) / 256)), dim3(256), 0, st, M.t, A, x, y,
		f_alpha, f_beta);
	if(M.n_chunks > 0) {
		hipLaunchKernelGGL((multiply_long_kernel<D>), dim3(unsigned(M.n_chunks)), dim3(64), 0, st, M.t, M.d_chunks.p(), A, x,
			M.d_partial.p());
		hipLaunchKernelGGL(multiply_long_finish_kernel, dim3(unsigned((M.n_long_rows * 8 + 63) / 64)), dim3(64), 0, st, M.t,
			M.d_long_rows.p(), M.n_long_rows, M.d_partial.p(), y, f_alpha, f_beta);
	}
}

void multiply_enqueue(const CMultiplyState &M, const double *A, const double *x, double *y, double f_alpha, double f_beta,
	hipStream_t st)
{
	switch(M.n_max_dim) {
	case 1: multiply_launch<1>(M, A, x, y, f_alpha, f_beta, st); break;
	case 2: multiply_launch<2>(M, A, x, y, f_alpha, f_beta, st); break;
	case 3: multiply_launch<3>(M, A, x, y, f_alpha, f_beta, st); break;
	case 4: multiply_launch<4>(M, A, x, y, f_alpha, f_beta, st); break;
	case 5: multiply_launch<5>(M, A, x, y, f_alpha, f_beta, st); break;
	case 6: multiply_launch<6>(M, A, x, y, f_alpha, f_beta, st); break;
	case 7: multiply_launch<7>(M, A, x, y, f_alpha, f_beta, st); break;
	case 8: multiply_launch<8>(M, A, x, y, f_alpha, f_beta, st); break;
	default:
		hipLaunchKernelGGL(multiply_generic_kernel, dim3(unsigned(M.t.n)), dim3(64), 0, st, M.t, A, x, y, f_alpha, f_beta);
	}
	SLAMPP_HIP_CHECK(hipGetLastError());
}

// ---- fixed-order reductions ----

// OP 0: sum of a_i b_i; 1: max of |a_i| (a NaN entry makes the result NaN)
template <int OP>
__device__ __forceinline__ double reduce_combine(double f_acc, double f_v)
{
	if(OP == 0)
		return f_acc + f_v;
	return (f_acc != f_acc || f_v <= f_acc)? f_acc : f_v; // (f_v NaN: the comparison fails and it is taken)
}

template <int OP>
__device__ __forceinline__ double reduce_workgroup(double f_acc) // 256 threads; the result in thread 0
{
	__shared__ double s_red[4];
	#pragma unroll
	for(int m = 1; m < 64; m <<= 1)
		f_acc = reduce_combine<OP>(f_acc, __shfl_xor(f_acc, m));
	if(threadIdx.x % 64 == 0)
		s_red[threadIdx.x / 64] = f_acc;
	__syncthreads();
	return reduce_combine<OP>(reduce_combine<OP>(s_red[0], s_red[1]), reduce_combine<OP>(s_red[2], s_red[3]));
}

template <int OP>
__global__ void __launch_bounds__(256)
reduce_first_kernel(const double *__restrict__ a, const double *__restrict__ b, int64_t n, double *partial)
{
	const int64_t n_stride = int64_t(gridDim.x) * 256;
	double f_acc = 0;
	for(int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += n_stride)
		f_acc = reduce_combine<OP>(f_acc, (OP == 0)? a[i] * b[i] : fabs(a[i]));
	f_acc = reduce_workgroup<OP>(f_acc);
	if(threadIdx.x == 0)
		partial[blockIdx.x] = f_acc;
}

template <int OP>
__global__ void __launch_bounds__(256)
reduce_second_kernel(const double *__restrict__ partial, int n_partials, double *out)
{
	double f_acc = 0;
	for(int i = threadIdx.x; i < n_partials; i += 256)
		f_acc = reduce_combine<OP>(f_acc, partial[i]);
	f_acc = reduce_workgroup<OP>(f_acc);
	if(threadIdx.x == 0)
		*out = f_acc;
}

template <int OP>
static void reduce_enqueue(const double *a, const double *b, int64_t n, double *partial, double *out, hipStream_t st)
{
	const int n_groups = int(std::min<int64_t>(reduce_MAX_PARTIALS, std::max<int64_t>(1, (n + 1023) / 1024))); // (of n alone)
	hipLaunchKernelGGL((reduce_first_kernel<OP>), dim3(n_groups), dim3(256), 0, st, a, b, n, partial);
	hipLaunchKernelGGL((reduce_second_kernel<OP>), dim3(1), dim3(256), 0, st, partial, n_groups, out);
	SLAMPP_HIP_CHECK(hipGetLastError());
}

void dot_enqueue(const double *p_a, const double *p_b, int64_t n, double *p_partials, double *p_out, hipStream_t stream)
{
	reduce_enqueue<0>(p_a, p_b, n, p_partials, p_out, stream);
}

void norm_inf_enqueue(const double *p_a, int64_t n, double *p_partials, double *p_out, hipStream_t stream)
{
	reduce_enqueue<1>(p_a, p_a, n, p_partials, p_out, stream);
}

// keep = x, and x += d unless an earlier step of this call was turned down (*p_stop != 0)
__global__ void __launch_bounds__(256)
refine_step_kernel(double *x, double *__restrict__ keep, const double *__restrict__ d, int64_t n, const double *__restrict__ p_stop)
{
	const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
	if(i < n) {
		const double f_x = x[i];
		keep[i] = f_x;
		if(*p_stop == 0)
			x[i] = f_x + d[i];
	}
}

// the step stands if it at least halved the residual norm (a NaN fails the comparison); otherwise x = keep, the norm
// reported is the one before the step and *p_stop is set.  p_next is not p_prev or p_trial, and nobody reads it or p_stop here
__global__ void __launch_bounds__(256)
refine_accept_kernel(double *x, const double *__restrict__ keep, int64_t n, const double *__restrict__ p_prev,
	const double *__restrict__ p_trial, double *p_next, double *p_stop)
{
	const int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x;
	const double f_prev = *p_prev, f_trial = *p_trial;
	const bool b_taken = 2 * f_trial <= f_prev;
	if(!b_taken && i < n)
		x[i] = keep[i];
	if(i == 0) {
		*p_next = (b_taken)? f_trial : f_prev;
		if(!b_taken)
			*p_stop = 1;
	}
}

void refine_step_enqueue(double *p_x, double *p_keep, const double *p_d, int64_t n, const double *p_stop, hipStream_t stream)
{
	hipLaunchKernelGGL(refine_step_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, stream, p_x, p_keep, p_d, n, p_stop);
	SLAMPP_HIP_CHECK(hipGetLastError());
}

void refine_accept_enqueue(double *p_x, const double *p_keep, int64_t n, const double *p_prev, const double *p_trial,
	double *p_next, double *p_stop, hipStream_t stream)
{
	hipLaunchKernelGGL(refine_accept_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, stream, p_x, p_keep, n, p_prev,
		p_trial, p_next, p_stop);
	SLAMPP_HIP_CHECK(hipGetLastError());
}

} // namespace slampp

// the row lists of the current structure, built at the first product after a set_structure
void slampp_hip_solver::Require_Multiply()
{
	if(p_mul && b_mul_valid && slampp::multiply_long_row_threshold(p_mul) == n_multiply_long_row)
		return;
	if(p_mul) {
		SLAMPP_HIP_CHECK(hipStreamSynchronize(stream)); // (a product enqueued earlier may still read the old lists)
		slampp::multiply_destroy(p_mul);
		p_mul = 0;
	}
	p_mul = slampp::multiply_setup(int64_t(cumsum.size()) - 1, cumsum, bcol_ptr, brow, n_multiply_long_row, stream);
	b_mul_valid = true;
}
