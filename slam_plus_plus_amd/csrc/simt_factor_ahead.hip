// simt_factor_ahead.hip -- the lane-per-task factor kernel (simt_kernel.hip: factor_simt_kernel) for launches that cannot fill
// the chip (C3's leaf stage: 592 waves on 1 024 SIMDs), where nothing but the wave itself hides its waits.
//
// factor_simt_kernel starts every column with the "touch" of the next column's Lambda blocks: loads whose sum is taken inside a
// loop of run-time length, so each of them is waited for (three serialized misses to HBM a column, and the first of the waits
// also drains the stores of the column before: one counter), and every line of Lambda is asked for twice, once by the touch and
// once by the load that uses it -- a trip to L2 in front of the row entries and one more in front of every block below the
// diagonal.  Nothing of this depends on what the kernel computes: Lambda and b are inputs of the step.  So here everything
// column ci + 1 reads of them is requested into a register set while column ci is factored, and column ci + 1 starts from
// registers.  A set: the stored triangle of Lambda's diagonal block, b_j, and the lane's half rows of the first AHEAD blocks
// below the diagonal (at C3 79 884 of 83 949 leaf columns have exactly two); a column's further blocks are loaded inside the
// column as before.  One set is in flight at a time: a column moves its set into the accumulators (a, y, acc) first, and the
// fetch of the next goes out behind the column's row entries, in front of the Cholesky and the inverse of the diagonal block
// -- some 330 dependent fp64 instructions with no load among them.  The loads of the column's own operands (L) further down
// queue behind the fetch, which by then has had that stretch of arithmetic to arrive.  No touches, no second request of a line.
//
// The operations and their order are factor_simt_kernel's because they are the same functions (simt_device.inl: row entries,
// Cholesky and inverse, forward substitution, a block below the diagonal, the Lambda load of the blocks a set does not hold);
// the selects on enc of a set's values are written here after simt_load_lambda_block's.  So is what every store writes: L,
// inv(L_jj), w and the flag are the same bits.  (Who stores the diagonal block differs: the lanes of a pair take half its columns each,
// where factor_simt_kernel leaves them to the first lane -- see there for why.)  Two lanes per task and even D only (the 8-byte loads of a half block stay apart; with one lane per task the
// compiler merges the loads of a set past what a wait can count).  One wave a SIMD: VGPRs and AGPRs up to the file, no scratch.
// Own translation unit (the register allocation of factor_simt_kernel moves with its neighbours: dense_tiles.hip says why).
#include <hip/hip_runtime.h>
#include "sparse_kernels.h"

#include <algorithm>

namespace slampp {

#include "simt_device.inl"

// what a column reads of the step's inputs
template <int D, int AHEAD>
struct TFactorAheadSet {
	double d[D][D];            // d[r][q], q <= r: element (q, r) of Lambda's stored diagonal block (the others are not loaded)
	double b[D];               // b_j
	double c[AHEAD][D / 2][D]; // c[k][i][q]: element (r0 + i, q) of the block k + 1 below the diagonal
};

// requests of one fetch (16-byte loads of the diagonal block's columns down to their diagonal element and of b_j, 8-byte loads
// of the half blocks) and stores of half a block: what the written-out waits count (simt_wait_imm, simt_device.inl)
template <int D, int AHEAD>
constexpr int factor_ahead_fetch_loads()
{
	int n = D / 2;
	for(int r = 0; r < D; ++ r)
		n += r / 2 + 1;
	return n + AHEAD * (D / 2) * D;
}
// (a half block's stores: per column D / 2 doubles, 16 bytes a store and one of 8 where D / 2 is odd; the diagonal block's: y_j and
// half the columns of L_jj.  The smaller of the two is what lies behind a fetch on every path to the next column's wait)
template <int D> constexpr int factor_ahead_half_block_stores() { return D * ((D / 2) / 2 + (D / 2) % 2); }
template <int D> constexpr int factor_ahead_diagonal_stores() { return D / 2 + (D / 2) * (D / 2); }
template <int D> constexpr int factor_ahead_newer_stores() { return (factor_ahead_half_block_stores<D>() < factor_ahead_diagonal_stores<D>())? factor_ahead_half_block_stores<D>() : factor_ahead_diagonal_stores<D>(); }

// The set stays where its loads put it until the column's wait has passed: an empty asm that wants every value in the accumulation
// half of the register file, which is where the allocator puts most of a set anyway -- without it the values were moved to
// the registers the next column reads them from at the column's end, behind a wait for everything
template <int D, int AHEAD>
__device__ __forceinline__ void factor_ahead_pin(TFactorAheadSet<D, AHEAD> &s)
{
	#pragma unroll
	for(int r = 0; r < D; ++ r) {
		#pragma unroll
		for(int q = 0; q < 2 * (r / 2 + 1); ++ q)
			asm volatile("" : "+a"(s.d[r][q]));
		asm volatile("" : "+a"(s.b[r]));
	}
	#pragma unroll
	for(int k = 0; k < AHEAD; ++ k) {
		#pragma unroll
		for(int i = 0; i < D / 2; ++ i) {
			#pragma unroll
			for(int q = 0; q < D; ++ q)
				asm volatile("" : "+a"(s.c[k][i][q]));
		}
	}
}

// Every fetch issues the same number of loads, whatever the column holds (backward_simt_ahead_kernel: a wait is "at most N
// operations outstanding", and N is what the compiler can prove of every path to it): a block the column does not have, or
// one that is fill-in, is a stand-in load from Lambda's first block, whose value the selects on enc discard.
// n_blk: the column's first block among the task's; nb: its blocks
template <int D, int W, int AHEAD>
__device__ __forceinline__ void factor_ahead_fetch(TFactorAheadSet<D, AHEAD> &s, int ci, int n_blk, int nb, int f_blk, int r0, const long long *T,
	const double *__restrict__ A, const double *__restrict__ b)
{
	{
		const long long enc = T[W * (f_blk + n_blk)];
		long long n_off = (enc < 0)? 0 : (enc >> 1);
		asm volatile("" : "+v"(n_off));
		const double *src = A + n_off;
		#pragma unroll
		for(int r = 0; r < D; ++ r) { // column r of the stored block: elements (0 .. r, r)
			#pragma unroll
			for(int i = 0; i <= r / 2; ++ i) {
				const double2 t = *reinterpret_cast<const double2*>(src + r * D + 2 * i);
				s.d[r][2 * i] = t.x;
				s.d[r][2 * i + 1] = t.y;
			}
		}
		load_column<D>(b + T[W * (4 * ci + 3)], s.b);
	}
	#pragma unroll
	for(int k = 0; k < AHEAD; ++ k) {
		const bool b_exists = k + 1 < nb; // (wave-uniform)
		const long long enc = T[W * (f_blk + n_blk + (b_exists? k + 1 : 0))];
		const bool b_trans = b_exists && enc >= 0 && (enc & 1) != 0;
		long long n_off = (b_exists && enc >= 0)? (enc >> 1) : 0;
		// element (r0 + i, q) of the block: stored at (r0 + i) + q D, or transposed at q + (r0 + i) D
		int n_row_stride = b_trans? D : 1, n_col_stride = b_trans? 1 : D;
		asm volatile("" : "+v"(n_off), "+v"(n_row_stride), "+v"(n_col_stride)); // (or the stand-ins are recognized as loads already made, and merged)
		const double *src = A + n_off + r0 * n_row_stride;
		#pragma unroll
		for(int i = 0; i < D / 2; ++ i) {
			#pragma unroll
			for(int q = 0; q < D; ++ q)
				s.c[k][i][q] = src[i * n_row_stride + q * n_col_stride];
		}
	}
	asm volatile("" ::: "memory"); // (the requests go out here, not where the scheduler would like them: next to their use)
}

// columns [n_half D / 2, (n_half + 1) D / 2) of m: m[r][q] -> p[r + q D]
template <int D>
__device__ __forceinline__ void store_half_columns(double *p, const double (&m)[D][D], int n_half)
{
	double *p_out = p + n_half * (D / 2) * D;
	#pragma unroll
	for(int q = 0; q < D / 2; ++ q) {
		#pragma unroll
		for(int r = 0; r < D; r += 2)
			*reinterpret_cast<double2*>(p_out + r + q * D) = double2{n_half? m[r][q + D / 2] : m[r][q], n_half? m[r + 1][q + D / 2] : m[r + 1][q]};
	}
}

// The column loop of one chunk -- a whole task a lane pair, or one segment of a split task: the one loop of both kernels below.
// P: the chunk's program (wave-uniform: scalar loads); T: field f of this lane's task at T[W f]; n_half: which half of the rows
// below the diagonal this lane takes; p_tm, n_tm: the clock samples of the wave that takes them (SIMT_TICK).  Returns whether
// a pivot was not positive.
template <int D, int W, bool b_linv, int AHEAD>
__device__ __forceinline__ bool factor_ahead_columns(const int32_t *P, const long long *T, const int n_half, const double *__restrict__ A, double *L, double *Linv,
	const double *__restrict__ b, double *w, long long *p_tm, int &n_tm)
{
	enum { DD = D * D, DH = D / 2 };
	const int r0 = n_half * DH;
	const int n_cols = P[0], n_blocks = P[1], n_ops = P[2];
	const int f_blk = 4 * n_cols, f_op = f_blk + n_blocks, f_y = f_op + n_ops;
	int pc = 4, blk0 = 0;
	bool b_bad = false;
	TFactorAheadSet<D, AHEAD> t_set;
	factor_ahead_fetch<D, W, AHEAD>(t_set, 0, 0, P[pc], f_blk, r0, T, A, b); // prologue: the first column, waited for right away
	__builtin_amdgcn_s_waitcnt(simt_wait_imm(0));
	factor_ahead_pin<D, AHEAD>(t_set); // (or the loads are moved past the wait, into the loop's preheader, and the loop is entered with the set pending)
	for(int ci = 0; ci < n_cols; ++ ci) {
		const int nb = P[pc], nr = P[pc + 1], n_touch = P[pc + 2];
		pc += 3;
		pc += n_touch;
		const long long l_base = T[W * (4 * ci)], linv_off = T[W * (4 * ci + 1)], cs_new = T[W * (4 * ci + 2)];
		// The one wait for the set, written out: everything but the newest requests has arrived.  Behind the fetch lie the stores of
		// the diagonal block and, of every block below it, operand loads (waited for where they were used: so was everything in
		// front of them, the set included) and the stores of half a block: those may still be on their way -- the column before is
		// not drained.  The compiler's own waits stay and add what correctness needs: with this one in front of them it adds none.
		__builtin_amdgcn_s_waitcnt(simt_wait_imm(factor_ahead_newer_stores<D>()));
		factor_ahead_pin<D, AHEAD>(t_set);
		double a[D][D], y[D], acc[AHEAD][DH][D]; // a: lower triangle of the diagonal block
		{
			// the diagonal block of Lambda: its upper triangle is what the reference's solvers consume; element (r, q), r >= q, is
			// stored element (q, r)
			const long long enc = T[W * (f_blk + blk0)];
			#pragma unroll
			for(int r = 0; r < D; ++ r) {
				#pragma unroll
				for(int q = 0; q < D; ++ q)
					a[r][q] = (q <= r && enc >= 0)? t_set.d[r][q] : 0.0;
			}
			#pragma unroll
			for(int r = 0; r < D; ++ r)
				y[r] = t_set.b[r];
			#pragma unroll
			for(int k = 0; k < AHEAD; ++ k) {
				const bool b_have = k + 1 < nb && T[W * (f_blk + blk0 + ((k + 1 < nb)? k + 1 : 0))] >= 0;
				#pragma unroll
				for(int i = 0; i < DH; ++ i) {
					#pragma unroll
					for(int q = 0; q < D; ++ q)
						acc[k][i][q] = b_have? t_set.c[k][i][q] : 0.0;
				}
			}
		}
		simt_row_entries<D, W>(a, y, pc, nr, f_op, f_y, P, T, L, w); // blocks L(j,c) of block row j
		SIMT_TICK(); // Lambda, row entries
		// the next column's set: requested here, where nothing but arithmetic follows for a while
		if(ci + 1 < n_cols) {
			asm volatile("" ::: "memory");
			factor_ahead_fetch<D, W, AHEAD>(t_set, ci + 1, blk0 + nb, P[pc_next_column(P, pc, nb, 0)], f_blk, r0, T, A, b);
		}
		double x[D][D]; // inv(L_jj)
		simt_cholesky_inverse<D>(a, x, b_bad);
		{
			double yn[D];
			simt_forward_substitution<D>(yn, a, x, y);
			// The lanes of a pair hold the same numbers: each stores half the columns of the diagonal block (and of its inverse), both
			// store y_j -- the same values to the same place.  No lane is masked out, so no path goes round these stores, and the
			// compiler can count them behind the fetch on every path to the next column's wait (with "if(n_half == 0)" around them it
			// skips them where no lane takes part, and the wait it proves is vmcnt(0))
			#pragma unroll
			for(int r = 0; r < D; r += 2)
				*reinterpret_cast<double2*>(w + cs_new + r) = double2{yn[r], yn[r + 1]};
			store_half_columns<D>(L + l_base, a, n_half);
			if constexpr(b_linv)
				store_half_columns<D>(Linv + linv_off, x, n_half);
		}
		SIMT_TICK(); // diagonal block
		// sub-diagonal blocks: L(i,j) = (Lambda(i,j) - sum L(i,c) L(j,c)^T) inv(L_jj)^T, each lane its DH rows of the block: the
		// first AHEAD of them from the set (the loop is unrolled: an accumulator indexed by a run-time number would be scratch)
		#pragma unroll
		for(int k = 0; k < AHEAD; ++ k) {
			if(k + 1 < nb) {
				const int np = P[pc ++];
				simt_update_pairs<D, W, 2>(acc[k], pc, np, f_op, r0, P, T, L);
				simt_block_product<D, 2>(acc[k], x, r0, L + l_base + (k + 1) * DD);
				SIMT_TICK(); // one sub-diagonal block
			}
		}
		for(int kb = AHEAD + 1; kb < nb; ++ kb) { // the blocks the set does not hold: Lambda from memory, as factor_simt_kernel
			const int np = P[pc ++];
			double acc_more[DH][D];
			simt_load_lambda_block<D, 2>(acc_more, T[W * (f_blk + blk0 + kb)], r0, A);
			simt_update_pairs<D, W, 2>(acc_more, pc, np, f_op, r0, P, T, L);
			simt_block_product<D, 2>(acc_more, x, r0, L + l_base + kb * DD);
			SIMT_TICK(); // one sub-diagonal block
		}
		blk0 += nb;
		// (what a lane loads in the following columns is what the lane itself has stored, or what an earlier launch
		// has: program order of one thread, no fence)
	}
	return b_bad;
}

template <int D, int W, int LPT, bool b_linv, int AHEAD> // (the arguments, programs, tables and LDS layout of factor_simt_kernel)
__global__ void __launch_bounds__(64)
factor_simt_kernel_ahead(const TSimtChunk *__restrict__ chunks, const int32_t *__restrict__ prog, const long long *__restrict__ tab,
	const double *__restrict__ A, double *L, double *Linv, const double *__restrict__ b, double *w, int *p_flag,
	long long *p_timing, TBatch t_batch)
{	{ const int64_t n_member = blockIdx.y; A += n_member * t_batch.a; L += n_member * t_batch.l; Linv = Linv? Linv + n_member * t_batch.linv : Linv; b += n_member * t_batch.b; w += n_member * t_batch.w; p_flag += n_member; } // (TBatch: sparse_kernels.h)

	static_assert(LPT == 2 && D % 2 == 0 && AHEAD >= 1, "two lanes per task, even block sizes");
	enum { DD = D * D, DH = D / 2 };
	extern __shared__ long long s_tab[]; // the chunk's table of per-lane offsets
	const TSimtChunk ch = chunks[blockIdx.x];
	{
		const int n_entries = (4 * prog[ch.prog_off] + prog[ch.prog_off + 1] + prog[ch.prog_off + 2] + prog[ch.prog_off + 3]) * W;
		simt_stage_table(s_tab, tab + ch.tab_off, n_entries, int(threadIdx.x));
		__syncthreads();
	}
	if(int(threadIdx.x) >= W * LPT)
		return; // (no barrier below)
	const int n_half = int(threadIdx.x) & 1; // which half of the rows below the diagonal this lane takes
	int n_tm = 0;
	long long *p_tm = simt_timing_begin(p_timing, n_tm); // development aid (SLAMPP_HIP_STAGE_TIMING)
	const bool b_bad = factor_ahead_columns<D, W, b_linv, AHEAD>(prog + ch.prog_off, s_tab + threadIdx.x / LPT, n_half, A, L, Linv, b, w, p_tm, n_tm);
	if(b_bad)
		atomicOr(p_flag, 1);
}

// The launch whose longest tasks set its duration (C3's leaves: the waves of five-column tasks are through at 38 us, those of
// eight-column tasks at 71 us, and most of the chip idles in between).  A leaf task is no chain: its branches are independent
// until they meet.  A workgroup of two waves runs three segments (TSimtBranchGroup, sparse_kernels.h): waves 0 and 1 the two
// bins of whole branch chains of one chunk of split tasks, side by side; behind the barrier wave 0 the join columns above them,
// the same tasks in the same lanes.  Chunks of whole tasks ride two to a workgroup and have no third segment.  The join columns
// read blocks and entries of w that wave 1 stored: both waves are in one CU (one vector cache), and the barrier with its
// workgroup-scope fence orders the stores in front of the loads.  A wave stages its segment's table into its own LDS region of
// n_region entries; the column loop is factor_simt_kernel_ahead's, and so is every bit stored.
template <int D, int W, bool b_linv, int AHEAD>
__global__ void __launch_bounds__(128)
factor_simt_kernel_branches(const TSimtBranchGroup *__restrict__ groups, const int32_t *__restrict__ prog, const long long *__restrict__ tab,
	const double *__restrict__ A, double *L, double *Linv, const double *__restrict__ b, double *w, int *p_flag,
	long long *p_timing, TBatch t_batch, int n_region)
{	{ const int64_t n_member = blockIdx.y; A += n_member * t_batch.a; L += n_member * t_batch.l; Linv = Linv? Linv + n_member * t_batch.linv : Linv; b += n_member * t_batch.b; w += n_member * t_batch.w; p_flag += n_member; } // (TBatch: sparse_kernels.h)

	static_assert(D % 2 == 0 && AHEAD >= 1 && W * 2 <= 64, "two lanes per task, even block sizes");
	extern __shared__ long long s_tab[]; // two regions: a wave's segment table of per-lane offsets
	const int n_wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6), n_lane = int(threadIdx.x) & 63; // (n_wave in a scalar register: what follows from it stays wave-uniform)
	long long *s_mine = s_tab + n_wave * n_region;
	int n_tm = 0;
	long long *p_tm = simt_timing_begin(p_timing, n_tm); // development aid (SLAMPP_HIP_STAGE_TIMING): the first wave of the workgroup
	bool b_bad = false;
	for(int n_pass = 0; n_pass < 2; ++ n_pass) { // the bins side by side, then the joins on wave 0
		const TSimtChunk ch = groups[blockIdx.x].seg[n_pass? 2 : n_wave];
		if(ch.n_tasks > 0 && (n_pass == 0 || n_wave == 0)) { // (wave-uniform)
			const int32_t *P = prog + ch.prog_off;
			const int n_entries = (4 * P[0] + P[1] + P[2] + P[3]) * W;
			simt_stage_table(s_mine, tab + ch.tab_off, n_entries, n_lane);
			__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); // (the region is this wave's own: its lanes' stores in front of its lanes' loads, no barrier)
			__builtin_amdgcn_wave_barrier();
			if(n_lane < W * 2) { // (idle lanes of a narrow wave go on to the barrier)
				const bool b_bad_here = factor_ahead_columns<D, W, b_linv, AHEAD>(P, s_mine + n_lane / 2, n_lane & 1, A, L, Linv, b, w, p_tm, n_tm);
				b_bad = b_bad || b_bad_here;
			}
		}
		if(n_pass == 0)
			__syncthreads(); // (what the bins stored of L, inv(L_jj) and w, in front of what the joins load)
	}
	if(b_bad)
		atomicOr(p_flag, 1);
}

template <int W>
static const void *p_Factor_Branches_Kernel(bool b_store_linv)
{
	return b_store_linv? reinterpret_cast<const void*>(&factor_simt_kernel_branches<6, W, true, SIMT_FACTOR_AHEAD>) :
		reinterpret_cast<const void*>(&factor_simt_kernel_branches<6, W, false, SIMT_FACTOR_AHEAD>);
}

static const void *p_Factor_Branches_Kernel(int n_dim, int n_width, bool b_store_linv)
{
	if(n_dim != 6)
		return 0;
	return (n_width == 16)? p_Factor_Branches_Kernel<16>(b_store_linv) : (n_width == 32)? p_Factor_Branches_Kernel<32>(b_store_linv) : 0;
}

bool factor_simt_branches_exists(int n_dim, int n_width)
{
	return p_Factor_Branches_Kernel(n_dim, n_width, false) != 0;
}

int factor_simt_branches_groups(int n_dim, int n_width, int n_lds_bytes)
{
	if(!factor_simt_branches_exists(n_dim, n_width) || n_lds_bytes <= 0)
		return 0;
	return std::min(simt_resident_workgroups(p_Factor_Branches_Kernel(n_dim, n_width, false), 128, n_lds_bytes),
		simt_resident_workgroups(p_Factor_Branches_Kernel(n_dim, n_width, true), 128, n_lds_bytes)); // (the smaller answer of the two instantiations)
}

bool launch_factor_simt_branches(const TSimtBranchGroup *groups, int n_groups, int n_width, int n_lds_bytes, const int32_t *prog, const int64_t *tab, int n_dim,
	const double *A, double *L, double *Linv, const double *b, double *w, int *p_flag, hipStream_t stream, long long *p_timing, const TBatch &t_batch)
{
	if(!factor_simt_branches_exists(n_dim, n_width) || n_groups <= 0 || n_lds_bytes <= 0 || n_lds_bytes % 16 != 0)
		return false;
	const long long *t = reinterpret_cast<const long long*>(tab);
	const int n_region = n_lds_bytes / 16; // (entries of one of the two regions)
#define BRANCHES_LAUNCH(W_, b_linv_) hipLaunchKernelGGL((factor_simt_kernel_branches<6, W_, b_linv_, SIMT_FACTOR_AHEAD>), dim3(n_groups, t_batch.n), dim3(128), n_lds_bytes, stream, \
	groups, prog, t, A, L, Linv, b, w, p_flag, p_timing, t_batch, n_region)
	if(n_width == 16) {
		if(Linv) BRANCHES_LAUNCH(16, true); else BRANCHES_LAUNCH(16, false);
	} else {
		if(Linv) BRANCHES_LAUNCH(32, true); else BRANCHES_LAUNCH(32, false);
	}
#undef BRANCHES_LAUNCH
	return true;
}

template <int W>
static const void *p_Factor_Ahead_Kernel(bool b_store_linv)
{
	return b_store_linv? reinterpret_cast<const void*>(&factor_simt_kernel_ahead<6, W, 2, true, SIMT_FACTOR_AHEAD>) :
		reinterpret_cast<const void*>(&factor_simt_kernel_ahead<6, W, 2, false, SIMT_FACTOR_AHEAD>);
}

static const void *p_Factor_Ahead_Kernel(int n_dim, int n_width, bool b_store_linv)
{
	if(n_dim != 6)
		return 0;
	return (n_width == 16)? p_Factor_Ahead_Kernel<16>(b_store_linv) : (n_width == 32)? p_Factor_Ahead_Kernel<32>(b_store_linv) : 0;
}

bool factor_simt_ahead_exists(int n_dim, int n_width)
{
	return p_Factor_Ahead_Kernel(n_dim, n_width, false) != 0;
}

int factor_simt_ahead_waves(int n_dim, int n_width, int n_lds_bytes)
{
	if(!factor_simt_ahead_exists(n_dim, n_width))
		return 0;
	return std::min(simt_resident_workgroups(p_Factor_Ahead_Kernel(n_dim, n_width, false), 64, n_lds_bytes),
		simt_resident_workgroups(p_Factor_Ahead_Kernel(n_dim, n_width, true), 64, n_lds_bytes)); // (the smaller answer of the two instantiations; a workgroup is one wave)
}

bool launch_factor_simt_ahead(const TSimtChunk *chunks, int n_chunks, int n_width, int n_lds_bytes, const int32_t *prog, const int64_t *tab, int n_dim,
	const double *A, double *L, double *Linv, const double *b, double *w, int *p_flag, hipStream_t stream, long long *p_timing, const TBatch &t_batch)
{
	if(!factor_simt_ahead_exists(n_dim, n_width))
		return false;
	const long long *t = reinterpret_cast<const long long*>(tab);
#define AHEAD_LAUNCH(W_, b_linv_) hipLaunchKernelGGL((factor_simt_kernel_ahead<6, W_, 2, b_linv_, SIMT_FACTOR_AHEAD>), dim3(n_chunks, t_batch.n), dim3(64), n_lds_bytes, stream, \
	chunks, prog, t, A, L, Linv, b, w, p_flag, p_timing, t_batch)
	if(n_width == 16) {
		if(Linv) AHEAD_LAUNCH(16, true); else AHEAD_LAUNCH(16, false);
	} else {
		if(Linv) AHEAD_LAUNCH(32, true); else AHEAD_LAUNCH(32, false);
	}
#undef AHEAD_LAUNCH
	return true;
}

} // namespace slampp

#include "preload.h"
SLAMPP_PRELOAD_UNIT(simt_factor_ahead) // (the handle's bring-up thread loads this unit's code object: capi.hip)
