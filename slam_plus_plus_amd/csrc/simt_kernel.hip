// simt_kernel.hip -- wide stages of the sparse block factorization, one *lane* per task.
//
// The stages at the bottom of a nested-dissection elimination tree hold thousands of tasks (at 100 000 poses: 15 894
// leaf subtrees of 4-8 columns, then 7 513 / 3 675 / 1 931 single separator columns), and those tasks come in a handful
// of shapes: the same number of columns, blocks, row entries and update pairs, referring to the same relative
// operands (at 100 000 poses 158 shapes, the six most frequent cover 87 % of the leaves).  The wave-per-task kernel
// (subtree_kernel.hip) spends about 600 wave-instructions on every 6 x 6 column with 36 of 64 lanes busy, most of
// them cross-lane traffic of the in-wave Cholesky (v_readlane, ds_bpermute, LDS tiles); it is bound by instruction
// issue at 6 % of the HBM roof.  Here 64 tasks of one shape share a wave and every lane runs
// the plain scalar algorithm on its own task: Cholesky, inverse and the block products are straight-line FMAs in
// registers, no lane ever talks to another, and one wave-instruction serves 64 columns (about 2 000 FMAs per column
// and lane = 31 wave-instructions per column instead of 600).  What differs between the lanes is data: where the
// blocks live.  So the *program* of a shape (column / block / pair counts and operand indices) is read with scalar
// loads, and a per-lane table holds the offsets (of the task's own blocks, of its Lambda blocks, of its operands).
// Operands go through the caches in the factor's ordinary layout: a lane reads its own 288-byte blocks with 16-byte
// loads (consecutive instructions of a lane walk down the same lines), and a block written by a lane is re-read by
// the same lane a column or two later.
//
// Arithmetic as in the other factor kernels (left-looking, one writer per block, fixed summation order); results
// differ from theirs in the last bits only through the order of the sums inside a 6-term dot product.
// The sums themselves -- row entries, Cholesky and inverse, the blocks below the diagonal, the backward pass's products and
// solve -- are written once, in simt_device.inl, for the kernels here and their forms in simt_factor_ahead.hip: that is why
// the forms store the same bits.  The kernels hold what differs between the forms: where the operands come from and when.
// Own translation unit (see dense_tiles.hip for why).
#include <hip/hip_runtime.h>
#include "sparse_kernels.h"

#include <algorithm>
#include <cstdio>

namespace slampp {

#include "simt_device.inl"

template <int D, int W, int LPT, bool b_linv> // W = tasks per wave, LPT = lanes per task (1, or 2 for even D: the lanes of a pair compute the
// diagonal block of a column both, and each half the rows of the blocks below it -- no traffic between them); b_linv: inv(L_jj)
// goes to memory as well (36 of a column's ~100 doubles at C3; the solve itself no longer reads it: backward_simt_kernel)
__global__ void __launch_bounds__(64)
factor_simt_kernel(const TSimtChunk *__restrict__ chunks, const int32_t *__restrict__ prog, const long long *__restrict__ tab,
	const double *__restrict__ A, double *L, double *Linv, const double *__restrict__ b, double *w, int *p_flag,
	long long *p_timing, TBatch t_batch)
{	{ const int64_t n_member = blockIdx.y; A += n_member * t_batch.a; L += n_member * t_batch.l; Linv = Linv? Linv + n_member * t_batch.linv : Linv; b += n_member * t_batch.b; w += n_member * t_batch.w; p_flag += n_member; } // (TBatch: sparse_kernels.h)

	enum { DD = D * D };
	extern __shared__ long long s_tab[]; // the chunk's table of per-lane offsets: fetched once, in one go, instead of a
	// trip to memory in front of every operand
	const TSimtChunk ch = chunks[blockIdx.x];
	{
		const int n_entries = (4 * prog[ch.prog_off] + prog[ch.prog_off + 1] + prog[ch.prog_off + 2] + prog[ch.prog_off + 3]) * W;
		simt_stage_table(s_tab, tab + ch.tab_off, n_entries, int(threadIdx.x));
		__syncthreads();
	}
	if(int(threadIdx.x) >= W * LPT)
		return; // (no barrier below)
	const int n_half = (LPT == 2)? int(threadIdx.x) & 1 : 0; // which half of the rows below the diagonal this lane takes
	enum { DH = (LPT == 2)? D / 2 : D };
	const int r0 = n_half * DH;
	int n_tm = 0;
	long long *p_tm = simt_timing_begin(p_timing, n_tm); // development aid (SLAMPP_HIP_STAGE_TIMING)
	const int32_t *P = prog + ch.prog_off;                 // wave-uniform: scalar loads
	const long long *T = s_tab + threadIdx.x / LPT;        // field f of this lane's task at T[W f]
	const int n_cols = P[0], n_blocks = P[1], n_ops = P[2];
	const int f_blk = 4 * n_cols, f_op = f_blk + n_blocks, f_y = f_op + n_ops;
	int pc = 4, blk0 = 0;
	bool b_bad = false;
	double f_touched = 0; // keeps the early loads alive
	for(int ci = 0; ci < n_cols; ++ ci) {
		const int nb = P[pc], nr = P[pc + 1], n_touch = P[pc + 2];
		pc += 3;
		pc += n_touch; // (the column's distinct operands, for a variant that requested their lines ahead: measured slower)
		// the Lambda blocks of the next column come from memory nobody has touched yet: one load per cache line of each goes
		// out now, a whole column of arithmetic ahead of their use
		if(ci + 1 < n_cols) {
			const int nb_next = P[pc_next_column(P, pc, nb, nr)];
			for(int kb = 0; kb < nb_next; ++ kb) {
				const long long enc = T[W * (f_blk + blk0 + nb + kb)];
				const double *p_src = A + ((enc < 0)? 0 : (enc >> 1));
				f_touched += p_src[0] + p_src[16] + p_src[DD - 1];
			}
		}
		const long long l_base = T[W * (4 * ci)], linv_off = T[W * (4 * ci + 1)], cs_new = T[W * (4 * ci + 2)],
			cs_src = T[W * (4 * ci + 3)];
		double a[D][D], y[D]; // a: lower triangle of the diagonal block
		{
			// the diagonal block of Lambda: its upper triangle is what the reference's solvers consume
			// (src/slam/LinearSolver_CholMod.cpp:57); element (r, q), r >= q, is stored element (q, r)
			const long long enc = T[W * (f_blk + blk0)];
			const double *src = A + ((enc < 0)? 0 : (enc >> 1));
			#pragma unroll
			for(int r = 0; r < D; ++ r) {
				double c[D];
				load_column<D>(src + r * D, c); // column r of the stored block: elements (0..D-1, r)
				#pragma unroll
				for(int q = 0; q < D; ++ q)
					a[r][q] = (q <= r && enc >= 0)? c[q] : 0.0;
			}
			load_column<D>(b + cs_src, y);
		}
		simt_row_entries<D, W>(a, y, pc, nr, f_op, f_y, P, T, L, w);
		SIMT_TICK(); // Lambda, row entries
		double x[D][D]; // inv(L_jj)
		simt_cholesky_inverse<D>(a, x, b_bad);
		{
			double yn[D];
			simt_forward_substitution<D>(yn, a, x, y);
			if(n_half == 0) { // (the lanes of a pair hold the same numbers)
				#pragma unroll
				for(int r = 0; r < D; ++ r)
					w[cs_new + r] = yn[r];
				store_block<D>(L + l_base, a);
				if constexpr(b_linv)
					store_block<D>(Linv + linv_off, x);
			}
		}
		SIMT_TICK(); // diagonal block
		// sub-diagonal blocks: L(i,j) = (Lambda(i,j) - sum L(i,c) L(j,c)^T) inv(L_jj)^T; with two lanes per task each lane
		// its DH rows of the block (inv(L_jj) is in its own registers: x above)
		for(int kb = 1; kb < nb; ++ kb) {
			const int np = P[pc ++];
			double acc[DH][D];
			simt_load_lambda_block<D, LPT>(acc, T[W * (f_blk + blk0 + kb)], r0, A);
			simt_update_pairs<D, W, LPT>(acc, pc, np, f_op, r0, P, T, L);
			double *p_out = L + l_base + kb * DD;
			if constexpr(D % 2 == 0)
				simt_block_product<D, LPT>(acc, x, r0, p_out);
			else {
				// Odd D (one lane per task, a whole block a lane, scalar stores) has no other form to agree with, and D = 7 fills the
				// VGPR file: through simt_block_product the same sums reach the scheduler in another order and the allocator parks
				// two to four more values in AGPRs (profiles/simt_shared_arith_isa.txt).  So these kernels keep the product as they
				// had it: out[r][q] = sum_{t <= q} acc[r][t] x[q][t], the sums simt_block_product writes.
				static_assert(LPT == 1, "odd D: one lane per task, the lane has all D rows of the block");
				#pragma unroll
				for(int q = 0; q < D; ++ q) {
					double out[D];
					#pragma unroll
					for(int r = 0; r < D; ++ r) {
						double sum = 0;
						#pragma unroll
						for(int t = 0; t <= q; ++ t)
							sum += acc[r][t] * x[q][t];
						out[r] = sum;
					}
					#pragma unroll
					for(int r = 0; r < D; ++ r)
						p_out[r + q * D] = out[r];
				}
			}
			SIMT_TICK(); // one sub-diagonal block
		}
		blk0 += nb;
		// (what a lane loads in the following columns is what the lane itself has stored, or what an earlier launch
		// has: program order of one thread, no fence)
	}
	if(b_bad || f_touched == 1.2345e301) // (never equal: the sum only has to be used)
		atomicOr(p_flag, 1);
}

bool launch_factor_simt(const TSimtChunk *chunks, int n_chunks, int n_width, int n_lds_bytes, const int32_t *prog, const int64_t *tab, int n_dim,
	const double *A, double *L, double *Linv, const double *b, double *w, int *p_flag, hipStream_t stream, long long *p_timing, const TBatch &t_batch,
	int n_ahead_waves, const TSimtBranchLaunch *p_branches)
{
	if(n_chunks <= 0)
		return true;
	const long long *t = reinterpret_cast<const long long*>(tab);
#define SIMT_LAUNCH(D_, W_, LPT_) do { if(Linv) hipLaunchKernelGGL((factor_simt_kernel<D_, W_, LPT_, true>), dim3(n_chunks, t_batch.n), dim3(64), n_lds_bytes, stream, chunks, prog, t, \
	A, L, Linv, b, w, p_flag, p_timing, t_batch); else hipLaunchKernelGGL((factor_simt_kernel<D_, W_, LPT_, false>), dim3(n_chunks, t_batch.n), dim3(64), n_lds_bytes, stream, chunks, prog, t, \
	A, L, Linv, b, w, p_flag, p_timing, t_batch); } while(0)
	// (two lanes per task where the block dimension is even and a wave holds at most 32 tasks)
#define SIMT_WIDTHS(D_) do { if(n_width == 16) { if(b_pairs && D_ % 2 == 0) SIMT_LAUNCH(D_, 16, (D_ % 2 == 0)? 2 : 1); else SIMT_LAUNCH(D_, 16, 1); } \
	else if(n_width == 32) { if(b_pairs && D_ % 2 == 0) SIMT_LAUNCH(D_, 32, (D_ % 2 == 0)? 2 : 1); else SIMT_LAUNCH(D_, 32, 1); } \
	else SIMT_LAUNCH(D_, 64, 1); } while(0)
	// Two lanes per task is a third more work per task (both lanes of a pair do the column's diagonal block) for half the
	// dependent chain of the blocks below it: it pays while the launch leaves the chip's SIMDs short of waves (C3: 497
	// waves on 1 024 SIMDs, 120 -> 100 us) and costs where they are full (a million poses: 716 -> 779 us).
	const int n_pairs_env = dev_knob("SLAMPP_HIP_DEV_SIMT_PAIRS", -1); // development aid (plan.h)
	const bool b_pairs = (n_pairs_env >= 0)? n_pairs_env != 0 : n_chunks <= 2048;
	// The fetch-ahead form (simt_factor_ahead.hip) runs at one wave a SIMD: it is for paired launches that fit the chip in one
	// round at that occupancy and so could not hide a wave's waits behind other waves anyway (C3's leaves: 592 waves).  Larger
	// launches -- a batch of eight, a million poses -- keep the kernel above, where the waits are hidden and registers would cost
	// residency.  Development aid (plan.h): 0 = never, 1 = wherever the form exists; the results are the same bits.
	const int n_ahead_env = dev_knob("SLAMPP_HIP_DEV_SIMT_FACTOR_AHEAD", -1);
	const int n_lpt = (b_pairs && n_dim % 2 == 0 && (n_width == 16 || n_width == 32))? 2 : 1;
	const bool b_ahead = n_lpt == 2 && factor_simt_ahead_exists(n_dim, n_width) &&
		((n_ahead_env >= 0)? n_ahead_env != 0 : int64_t(n_chunks) * std::max<int64_t>(t_batch.n, 1) <= n_ahead_waves);
	// The two-wave form (simt_factor_ahead.hip: factor_simt_kernel_branches) shortens the launch where its longest tasks set its
	// duration and everything else is through long before them (C3's leaves): the launch must be one the fetch-ahead form would
	// take, fit one round of the two-wave form, have tasks longer than T* columns, the longest chain a wave then walks -- and
	// be of a stage of at least 2 048 tasks, the size from which the analysis chooses the lane kernels by itself (below it only
	// option simt = 1 gets here).  Development aid (plan.h): 0 = never, 1 = wherever the stage has records; the same bits.
	const int n_branches_env = dev_knob("SLAMPP_HIP_DEV_SIMT_FACTOR_BRANCHES", -1);
	const bool b_branches = p_branches && p_branches->n_groups > 0 && n_lpt == 2 && factor_simt_branches_exists(n_dim, n_width) &&
		((n_branches_env >= 0)? n_branches_env != 0 : b_ahead && int64_t(p_branches->n_groups) * std::max<int64_t>(t_batch.n, 1) <= p_branches->n_round_groups &&
		p_branches->n_tstar < p_branches->n_longest_task && p_branches->n_stage_tasks >= 2048);
	if(b_branches) {
		if(p_timing)
			fprintf(stderr, "stage_timing lane-per-task factor branches launch: %d workgroups of two waves, %d split chunks, %d whole chunks, width %d, block size %d, %d members\n",
				p_branches->n_groups, p_branches->n_split_chunks, p_branches->n_whole_chunks, n_width, n_dim, int(t_batch.n));
		return launch_factor_simt_branches(p_branches->groups, p_branches->n_groups, n_width, p_branches->n_lds_bytes, prog, tab, n_dim, A, L, Linv, b, w, p_flag,
			stream, p_timing, t_batch);
	}
	if(p_timing) // (development aid SLAMPP_HIP_STAGE_TIMING: which form the launch takes, for the tests)
		fprintf(stderr, "stage_timing lane-per-task factor launch: %d chunks, width %d, block size %d, %d members, LPT %d, %s\n", n_chunks, n_width, n_dim,
			int(t_batch.n), n_lpt, b_ahead? "fetch ahead" : "fetch by column");
	if(b_ahead)
		return launch_factor_simt_ahead(chunks, n_chunks, n_width, n_lds_bytes, prog, tab, n_dim, A, L, Linv, b, w, p_flag, stream, p_timing, t_batch);
	switch(n_dim) {
	case 3:
		SIMT_WIDTHS(3);
		return true;
	case 6:
		SIMT_WIDTHS(6);
		return true;
	case 7:
		SIMT_WIDTHS(7);
		return true;
	default:
		return false;
	}
#undef SIMT_WIDTHS
#undef SIMT_LAUNCH
}

// Backward substitution of the same tasks, one lane per task: x_j = L_jj^-T (y_j - sum_i L(i,j)^T x_i), columns last to first.
// The wave-per-task kernel (backward_stage_kernel) pays a trip to memory per column with 36 lanes busy, 15 894 workgroups for
// C3's leaf subtrees (40 us); here a lane walks its task's columns with its own blocks, the next column's lines requested a
// column ahead, and solves with L_jj^T itself (six dependent steps, reciprocals taken before the chain) -- inv(L_jj) is not
// read, which is what lets the factorization stop writing it.  x of rows inside the task is what the lane stored a moment
// ago (program order of one thread), x of rows above it what earlier launches stored.
template <int D, int W>
__global__ void __launch_bounds__(64)
backward_simt_kernel(const TSimtChunk *__restrict__ chunks, const int32_t *__restrict__ prog, const long long *__restrict__ tab,
	const double *__restrict__ L, double *w, double *x_out, TBatch t_batch)
{	{ const int64_t n_member = blockIdx.y; L += n_member * t_batch.l; w += n_member * t_batch.w; x_out += n_member * t_batch.b; } // (TBatch: sparse_kernels.h)

	enum { DD = D * D };
	extern __shared__ long long s_tab[];
	const TSimtChunk ch = chunks[blockIdx.x];
	const int32_t *P = prog + ch.prog_off; // wave-uniform: scalar loads
	const int n_cols = P[0], n_below = P[1];
	{
		const int n_entries = (3 * n_cols + n_below) * W;
		simt_stage_table(s_tab, tab + ch.tab_off, n_entries, int(threadIdx.x));
		__syncthreads();
	}
	if(int(threadIdx.x) >= W)
		return; // (no barrier below)
	const long long *T = s_tab + threadIdx.x;
	// x of the task's own columns stays in LDS (round 6): a column's x is what the columns before it in the task multiply their
	// blocks with, and through memory that was a store and a load of the same thread through L2 per column -- the longest
	// waits of a kernel that waits 84 % of its time (tools/pmc_waits.sh c3).  Rows outside the task (the separators above,
	// solved by earlier launches) still come from w.  P[2 + n_cols + b]: which of the task's columns the row of block b is, or -1.
	double *s_x = reinterpret_cast<double*>(s_tab + (3 * n_cols + n_below) * W) + threadIdx.x;
	const int32_t *p_local = P + 2 + n_cols;
	int n_blk_end = n_below;
	double f_touched = 0;
	for(int ci = n_cols - 1; ci >= 0; -- ci) {
		const int nb = P[2 + ci];
		const long long l_base = T[W * (3 * ci)], cs_new = T[W * (3 * ci + 1)], cs_src = T[W * (3 * ci + 2)];
		const int n_blk0 = n_blk_end - (nb - 1);
		double acc[D], a[D][D];
		load_column<D>(w + cs_new, acc); // y_j
		load_block<D>(L + l_base, a);    // a[q][r] = L_jj(r, q)
		// The blocks of the column after next: a load per cache line, two columns of arithmetic ahead of their use -- and BEHIND
		// this column's own first loads (round 6).  Loads come back in the order they were issued (one counter): requested in
		// front of the column's own loads, as they were, the touches -- misses all the way to HBM -- were what every column's own,
		// long-arrived data waited behind.  Two columns ahead, because the next column's own loads queue behind these.
		asm volatile("" ::: "memory");
		double f_touch_now = 0;
		if(ci > 1 || (ci == n_cols - 1 && ci > 0)) {
			const int c_first = (ci > 1)? ci - 2 : ci - 1, c_last = (ci == n_cols - 1)? ci - 1 : c_first; // (the first column handled touches both)
			for(int c = c_last; c >= c_first; -- c) {
				const int nb_next = P[2 + c];
				const double *p_next = L + T[W * (3 * c)];
				for(int kb = 0; kb < nb_next; ++ kb)
					f_touch_now += p_next[kb * DD] + p_next[kb * DD + 16] + p_next[kb * DD + DD - 1];
			}
		}
		asm volatile("" ::: "memory");
		double rd[D];
		#pragma unroll
		for(int q = 0; q < D; ++ q)
			rd[q] = simt_refined_rcp(a[q][q]);
		for(int kb = 1; kb < nb; ++ kb) {
			const long long xcs = T[W * (3 * n_cols + n_blk0 + kb - 1)];
			const int n_local = p_local[n_blk0 + kb - 1]; // (wave-uniform)
			double c[D][D], xi[D];
			load_block<D>(L + l_base + kb * DD, c); // c[q][r] = L(i,j)(r, q)
			if(n_local >= 0)
				simt_local_x<D, W>(xi, s_x, n_local);
			else
				load_column<D>(w + xcs, xi);
			simt_backward_block<D>(acc, c, xi);
		}
		double x[D];
		simt_solve_transposed<D>(x, acc, a, rd);
		simt_store_local_x<D, W>(s_x, ci, x);
		f_touched += f_touch_now; // (used here: nothing of this column waits for the touches)
		simt_store_x<D>(w + cs_new, x_out + cs_src, x);
		n_blk_end = n_blk0;
	}
	if(f_touched == 1.2345e301) // (never: the sum only has to be used)
		w[0] = f_touched;
}

// The same substitution for launches that cannot fill the chip (C3's leaf stage: 592 waves on 1 024 SIMDs), where nothing but
// the wave itself hides its waits.  backward_simt_kernel pays four to six dependent trips to memory a column: its touches are
// loads whose sum is taken inside a loop of run-time length, so each of them is waited for, and the blocks below the diagonal
// come one per wait.  Nothing a column reads from memory depends on what the kernel computes (L is read-only, y_j and x of the
// rows outside the task are earlier launches' stores, x of the task's own columns travels through LDS), so here everything
// column ci - 1 needs is requested into a second register set before column ci is solved out of the first, and the wait of a
// column is for loads a whole column old, with the newer ones still in flight.  A set: y_j, L_jj, the first SIMT_BWD_AHEAD
// blocks below it and x of one row outside the task -- the first such row among those blocks; at C3 nearly every column has two
// blocks below its diagonal, one row inside the task and one outside.  A second outside row among them (the last column of a
// task) has its x fetched in the column, and waited for.  The column loop is unrolled by two, so the two sets stay in fixed
// registers (108 doubles each at D = 6 with two blocks: 512 registers in all, one wave a SIMD, no scratch; an x per block, 114
// doubles a set, spilled -- DESIGN.md section 10).  Columns with more blocks fetch the rest themselves, SIMT_BWD_AHEAD at a time
// into the set they are solving from, all before the first product: one more trip, and this one is waited for.  The arithmetic,
// its order and every store are backward_simt_kernel's, by way of the same functions of simt_device.inl (the solve with L_jj^T
// excepted: see bwd_ahead_solve): the results are the same bits.  No touches.
template <int D, int AHEAD>
struct TBwdAheadSet {
	double y[D], a[D][D], c[AHEAD][D][D], xs[D]; // xs: x of the first of those blocks' rows that lies outside the task; a[q][r] = L_jj(r, q), c[k][q][r] = L(i_k,j)(r, q)
	int nb, n_blk0; // (the column's offsets are read from the LDS table again where they are needed: registers) blocks of the column; position of its first sub-diagonal block among the task's
	int n_xk; // the block xs belongs to, or -1
	int n_local[AHEAD]; // which of the task's columns the row of block k + 1 is, or -1 (wave-uniform, as nb)
};

// Every fetch issues the same number of loads, whatever the column holds: a wait is written as "at most N loads outstanding",
// loads return in the order they went out, and N is what the compiler can prove of every path to the wait -- with a load count
// that followed nb and the rows' places it proved little (vmcnt(0) to (17) with 57 newer loads in flight: the newer column's
// trip exposed after all).  So a block the column does not have is the diagonal block once more (lines just requested), and a
// column with no row outside the task among its blocks reads its own y_j a second time for xs.
template <int D, int W, int AHEAD>
__device__ __forceinline__ void bwd_ahead_fetch(TBwdAheadSet<D, AHEAD> &s, int ci, int n_blk_end, int n_cols, const int32_t *P, const int32_t *p_local,
	const long long *T, const double *__restrict__ L, const double *w)
{
	enum { DD = D * D };
	s.nb = P[2 + ci];
	const long long l_base = T[W * (3 * ci)];
	s.n_blk0 = n_blk_end - (s.nb - 1);
	load_column<D>(w + T[W * (3 * ci + 1)], s.y); // y_j
	load_lower<D>(L + l_base, s.a);
	s.n_xk = -1;
	int n_x_field = 3 * ci + 1;
	#pragma unroll
	for(int k = 0; k < AHEAD; ++ k) {
		const bool b_have = k + 1 < s.nb; // (wave-uniform)
		s.n_local[k] = b_have? p_local[s.n_blk0 + k] : 0;
		if(b_have && s.n_local[k] < 0 && s.n_xk < 0) {
			s.n_xk = k;
			n_x_field = 3 * n_cols + s.n_blk0 + k;
		}
		int n_blk_off = b_have? (k + 1) * DD : 0;
		asm volatile("" : "+s"(n_blk_off)); // (or the stand-ins are recognized as the loads above, dropped, and their values copied: waits again)
		load_block<D>(L + l_base + n_blk_off, s.c[k]);
	}
	asm volatile("" : "+s"(n_x_field));
	load_column<D>(w + T[W * n_x_field], s.xs);
	asm volatile("" ::: "memory"); // (the requests go out here, not where the scheduler would like them: next to their use)
}

// requests of one fetch (even D: 16-byte loads, of L_jj those that hold an element of its lower triangle: load_lower) and
// stores of one solve: what the written-out waits count (simt_wait_imm, simt_device.inl)
template <int D, int AHEAD>
constexpr int bwd_ahead_fetch_loads()
{
	if(D % 2 != 0)
		return D + D * (D + 1) / 2 + AHEAD * (D * D) + D;
	int n = D / 2;
	for(int q = 0; q < D; ++ q)
		n += (D - (q & ~1)) / 2;
	return n + AHEAD * (D * D / 2) + D / 2;
}
template <int D> constexpr int bwd_ahead_solve_stores() { return (D % 2 == 0)? D : 2 * D; }

template <int D, int W, int AHEAD, int N_NEWER /* vector memory operations issued since the set's fetch, at the least */,
	bool b_slots = false /* the columns are a segment of a task (backward_simt_kernel_branches): x goes to LDS at p_slot[ci], the column's place in the whole task */>
__device__ __forceinline__ void bwd_ahead_solve(TBwdAheadSet<D, AHEAD> &s, int ci, int n_cols, const int32_t *p_local, const long long *T, double *s_x,
	const double *__restrict__ L, double *w, double *x_out, const int32_t *p_slot = 0)
{
	enum { DD = D * D };
	// The one wait of the column, written out: everything older than the N_NEWER newest requests -- this set -- has arrived.  The
	// compiler's own waits stay (it adds what correctness needs), but where paths of different load counts meet, behind the loop
	// of the remaining blocks, it no longer finds this set pending and asks for nothing: it asked for vmcnt(1) there.
	__builtin_amdgcn_s_waitcnt(simt_wait_imm(N_NEWER));
	#pragma unroll
	for(int q = 0; q < D; ++ q) // the reciprocals take the diagonal's place (registers)
		s.a[q][q] = simt_refined_rcp(s.a[q][q]);
	double acc[D];
	#pragma unroll
	for(int q = 0; q < D; ++ q)
		acc[q] = s.y[q];
	#pragma unroll
	for(int k = 0; k < AHEAD; ++ k) {
		if(k + 1 < s.nb) {
			double xi[D];
			if(s.n_local[k] >= 0) // a row inside the task: x from LDS
				simt_local_x<D, W>(xi, s_x, s.n_local[k]);
			else if(s.n_xk == k) {
				#pragma unroll
				for(int r = 0; r < D; ++ r)
					xi[r] = s.xs[r];
			} else { // a second row outside the task: fetched here, and waited for
				load_column<D>(w + T[W * (3 * n_cols + s.n_blk0 + k)], xi);
				__builtin_amdgcn_s_waitcnt(simt_wait_imm(0));
			}
			simt_backward_block<D>(acc, s.c[k], xi);
		}
	}
	const long long l_base = (s.nb > AHEAD + 1)? T[W * (3 * ci)] : 0;
	for(int kb = AHEAD + 1; kb < s.nb; kb += AHEAD) {
		double xr[AHEAD][D]; // the blocks the set did not hold: AHEAD of them a trip, into the set's own registers (their first tenants are used up)
		#pragma unroll
		for(int i = 0; i < AHEAD; ++ i) {
			if(kb + i < s.nb) {
				load_block<D>(L + l_base + (kb + i) * DD, s.c[i]);
				const int n_local = p_local[s.n_blk0 + kb + i - 1];
				if(n_local >= 0)
					simt_local_x<D, W>(xr[i], s_x, n_local);
				else
					load_column<D>(w + T[W * (3 * n_cols + s.n_blk0 + kb + i - 1)], xr[i]);
			}
		}
		asm volatile("" ::: "memory"); // (all of them requested before the first product)
		__builtin_amdgcn_s_waitcnt(simt_wait_imm(0)); // (written out for the same reason: no path leaves this loop with a request of its own pending)
		#pragma unroll
		for(int i = 0; i < AHEAD; ++ i) {
			if(kb + i < s.nb)
				simt_backward_block<D>(acc, s.c[i], xr[i]);
		}
	}
	double x[D];
	// (the solve of simt_solve_transposed, simt_device.inl, written out: with the reciprocals on s.a's diagonal the helper needs them in
	// an array of their own or behind a pointer, and either form moved this kernel's waits -- profiles/simt_shared_arith_isa.txt)
	#pragma unroll
	for(int q = D - 1; q >= 0; -- q) {
		double sum = acc[q];
		#pragma unroll
		for(int r = q + 1; r < D; ++ r)
			sum -= s.a[q][r] * x[r];
		x[q] = sum * s.a[q][q];
	}
	simt_store_local_x<D, W>(s_x, b_slots? p_slot[ci] : ci, x);
	const long long cs_new = T[W * (3 * ci + 1)], cs_src = T[W * (3 * ci + 2)];
	simt_store_x<D>(w + cs_new, x_out + cs_src, x);
}

// The columns of a chunk behind the prologue fetch (t_even holds the last column), last to first: the one loop of both kernels
// below.  b_slots, p_slot: as bwd_ahead_solve
template <int D, int W, int AHEAD, bool b_slots>
__device__ __forceinline__ void bwd_ahead_columns(TBwdAheadSet<D, AHEAD> &t_even, TBwdAheadSet<D, AHEAD> &t_odd, int n_cols, const int32_t *P, const int32_t *p_local,
	const int32_t *p_slot, const long long *T, double *s_x, const double *__restrict__ L, double *w, double *x_out)
{
	enum { N_FETCH = bwd_ahead_fetch_loads<D, AHEAD>(), N_STORES = bwd_ahead_solve_stores<D>() };
	int ci = n_cols - 1;
	for(; ci >= 2; ci -= 2) { // steady state: every solve with one fetch in front of it
		bwd_ahead_fetch<D, W, AHEAD>(t_odd, ci - 1, t_even.n_blk0, n_cols, P, p_local, T, L, w);
		bwd_ahead_solve<D, W, AHEAD, N_FETCH, b_slots>(t_even, ci, n_cols, p_local, T, s_x, L, w, x_out, p_slot); // (in the first round no store lies between the two fetches)
		bwd_ahead_fetch<D, W, AHEAD>(t_even, ci - 2, t_odd.n_blk0, n_cols, P, p_local, T, L, w);
		bwd_ahead_solve<D, W, AHEAD, N_STORES + N_FETCH, b_slots>(t_odd, ci - 1, n_cols, p_local, T, s_x, L, w, x_out, p_slot);
	}
	if(ci == 1) { // epilogue: the columns left (t_even holds column ci), the last of them with nothing to fetch
		bwd_ahead_fetch<D, W, AHEAD>(t_odd, 0, t_even.n_blk0, n_cols, P, p_local, T, L, w);
		bwd_ahead_solve<D, W, AHEAD, N_FETCH, b_slots>(t_even, 1, n_cols, p_local, T, s_x, L, w, x_out, p_slot);
		bwd_ahead_solve<D, W, AHEAD, N_STORES, b_slots>(t_odd, 0, n_cols, p_local, T, s_x, L, w, x_out, p_slot);
	} else
		bwd_ahead_solve<D, W, AHEAD, 0, b_slots>(t_even, 0, n_cols, p_local, T, s_x, L, w, x_out, p_slot);
}

template <int D, int W, int AHEAD>
__global__ void __launch_bounds__(64)
backward_simt_ahead_kernel(const TSimtChunk *__restrict__ chunks, const int32_t *__restrict__ prog, const long long *__restrict__ tab,
	const double *__restrict__ L, double *w, double *x_out, TBatch t_batch)
{	{ const int64_t n_member = blockIdx.y; L += n_member * t_batch.l; w += n_member * t_batch.w; x_out += n_member * t_batch.b; } // (TBatch: sparse_kernels.h)

	extern __shared__ long long s_tab[];
	const TSimtChunk ch = chunks[blockIdx.x];
	const int32_t *P = prog + ch.prog_off; // wave-uniform: scalar loads
	const int n_cols = P[0], n_below = P[1];
	{
		const int n_entries = (3 * n_cols + n_below) * W;
		simt_stage_table(s_tab, tab + ch.tab_off, n_entries, int(threadIdx.x));
		__syncthreads();
	}
	if(int(threadIdx.x) >= W)
		return; // (no barrier below)
	const long long *T = s_tab + threadIdx.x;
	double *s_x = reinterpret_cast<double*>(s_tab + (3 * n_cols + n_below) * W) + threadIdx.x; // x of the task's own columns (backward_simt_kernel)
	const int32_t *p_local = P + 2 + n_cols;
	TBwdAheadSet<D, AHEAD> t_even, t_odd; // (two named sets and a loop unrolled by two: an index into an array of sets would be scratch)
	bwd_ahead_fetch<D, W, AHEAD>(t_even, n_cols - 1, n_below, n_cols, P, p_local, T, L, w); // prologue: the last column
	bwd_ahead_columns<D, W, AHEAD, false>(t_even, t_odd, n_cols, P, p_local, 0, T, s_x, L, w, x_out);
}

// The fetch-ahead substitution for the launch whose longest tasks set its duration (C3's leaves: 592 one-wave workgroups on
// 1 024 SIMDs, the 30 % of the tasks with six to eight columns finish alone).  Backward substitution runs a task's tree from the
// top: the join columns first, then the two bins of whole branch chains (sparse_records.h: simt_task_segments()), which no longer
// depend on each other.  A workgroup of two waves runs one record (TSimtBranchGroup): wave 0 the joins (seg[2]), behind the one
// barrier waves 0 and 1 the bins (seg[0], seg[1]), the same tasks in the same lanes.  The bins exchange nothing through memory:
// x of the task's own columns is in LDS at the column's place in the whole task (the segment programs carry it: p_slot), the
// "which column" entries of a segment's rows stay in the task's numbering, and x of rows outside the task is earlier launches'.
// Chunks of whole tasks ride two to a record, as seg[0] and seg[1] with no joins, and then each wave has an x region of its own.
// LDS: three table regions of n_tab_region entries (seg[0], seg[1], seg[2]: every wave stages what it reads itself, all at the
// start), then two x regions of n_x_region doubles (a split record uses the first only).  One barrier, reached by every thread:
// idle lanes of a narrow chunk, a wave without a segment and the odd whole chunk without a partner included; no return in front
// of it.  Per column the operations and their order are backward_simt_ahead_kernel's (bwd_ahead_fetch, bwd_ahead_solve, the one
// column loop bwd_ahead_columns): the same bits.  (Wave 1 waits at the barrier with nothing requested: a first set fetched in
// front of the barrier and carried across it costs 324 bytes of scratch a lane -- the two sets fill the register file, and the
// set then has to sit in the same registers on both sides.  DESIGN.md section 10.)
template <int D, int W, int AHEAD>
__global__ void __launch_bounds__(128)
backward_simt_kernel_branches(const TSimtBranchGroup *__restrict__ groups, const int32_t *__restrict__ prog, const long long *__restrict__ tab,
	const double *__restrict__ L, double *w, double *x_out, TBatch t_batch, int n_tab_region, int n_x_region)
{	{ const int64_t n_member = blockIdx.y; L += n_member * t_batch.l; w += n_member * t_batch.w; x_out += n_member * t_batch.b; } // (TBatch: sparse_kernels.h)

	extern __shared__ long long s_tab[];
	const int n_wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6), n_lane = int(threadIdx.x) & 63; // (n_wave in a scalar register: what follows from it stays wave-uniform)
	const TSimtBranchGroup &r_group = groups[blockIdx.x];
	const bool b_shared_x = r_group.seg[2].n_tasks > 0; // (a record of split tasks: one x region for the task, written by both waves)
	for(int k = n_wave; k < 3; k += 2) { // wave 0: the tables of seg[0] and seg[2], wave 1: of seg[1]
		const TSimtChunk ch = r_group.seg[k];
		if(ch.n_tasks > 0) { // (wave-uniform)
			const int32_t *P = prog + ch.prog_off;
			simt_stage_table(s_tab + k * n_tab_region, tab + ch.tab_off, (3 * P[0] + P[1]) * W, n_lane);
		}
	}
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); // (the regions a wave reads are its own: its lanes' stores in front of its lanes' loads, no barrier)
	__builtin_amdgcn_wave_barrier();
	TBwdAheadSet<D, AHEAD> t_even, t_odd; // (as backward_simt_ahead_kernel)
	t_even.nb = t_even.n_blk0 = t_even.n_xk = 0; // (see between the two regions below)
	#pragma unroll
	for(int i = 0; i < AHEAD; ++ i)
		t_even.n_local[i] = 0;
	const bool b_my_lane = (int(threadIdx.x) & 63) < W; // (idle lanes of a narrow wave and a wave without a segment go on to the barrier)
	double *s_x = reinterpret_cast<double*>(s_tab + 3 * n_tab_region) + (b_shared_x? 0 : n_wave * n_x_region) + n_lane;
	{ // wave 0: the joins
		const TSimtChunk ch = r_group.seg[2];
		if(ch.n_tasks > 0 && !n_wave && b_my_lane) {
			const int32_t *P = prog + ch.prog_off; // n_cols, n_below, nb per column, per block which of the task's columns its row is, per column its place in the task
			const int n_cols = P[0], n_below = P[1];
			const long long *T = s_tab + 2 * n_tab_region + n_lane;
			const int32_t *p_local = P + 2 + n_cols;
			bwd_ahead_fetch<D, W, AHEAD>(t_even, n_cols - 1, n_below, n_cols, P, p_local, T, L, w); // prologue: the last column
			bwd_ahead_columns<D, W, AHEAD, true>(t_even, t_odd, n_cols, P, p_local, p_local + n_below, T, s_x, L, w, x_out);
		}
	}
	// What a set holds of the program (wave-uniform) leaves the region above, which only the chunk's lanes of wave 0 enter, in
	// vector registers.  The region below writes all of it anew, so nothing here changes a result; but the two sets fill the
	// register file, and with those words left where they are the kernel needs 20 bytes of scratch a lane, with them back in
	// scalar registers none (tests/test_simt_bwd_branches_resources.py)
	t_even.nb = __builtin_amdgcn_readfirstlane(t_even.nb);
	t_even.n_blk0 = __builtin_amdgcn_readfirstlane(t_even.n_blk0);
	t_even.n_xk = __builtin_amdgcn_readfirstlane(t_even.n_xk);
	#pragma unroll
	for(int i = 0; i < AHEAD; ++ i)
		t_even.n_local[i] = __builtin_amdgcn_readfirstlane(t_even.n_local[i]);
	__syncthreads(); // (x of the joins, in LDS, in front of the bins' loads of it)
	{ // both waves: their bins, or their chunks of whole tasks
		const TSimtChunk ch = r_group.seg[n_wave];
		if(ch.n_tasks > 0 && b_my_lane) {
			const int32_t *P = prog + ch.prog_off;
			const int n_cols = P[0], n_below = P[1];
			const long long *T = s_tab + (n_wave * n_tab_region - n_wave * 64) + int(threadIdx.x); // (= region n_wave + n_lane, from threadIdx.x itself: a register less)
			const int32_t *p_local = P + 2 + n_cols;
			bwd_ahead_fetch<D, W, AHEAD>(t_even, n_cols - 1, n_below, n_cols, P, p_local, T, L, w);
			bwd_ahead_columns<D, W, AHEAD, true>(t_even, t_odd, n_cols, P, p_local, p_local + n_below, T, s_x, L, w, x_out);
		}
	}
}

// the fetch-ahead form exists for the block sizes listed here (which compile without scratch)
template <int D> struct TBwdAheadDim { enum { b_have = (D == 6) }; };

template <int D, int W>
static const void *p_Backward_Ahead_Kernel()
{
	if constexpr(TBwdAheadDim<D>::b_have)
		return reinterpret_cast<const void*>(&backward_simt_ahead_kernel<D, W, SIMT_BWD_AHEAD>);
	else
		return 0;
}

static const void *p_Backward_Ahead_Kernel(int n_dim, int n_width)
{
#define BWD_AHEAD_WIDTHS(D_) return (n_width == 16)? p_Backward_Ahead_Kernel<D_, 16>() : (n_width == 32)? p_Backward_Ahead_Kernel<D_, 32>() : p_Backward_Ahead_Kernel<D_, 64>()
	switch(n_dim) {
	case 3:
		BWD_AHEAD_WIDTHS(3);
	case 6:
		BWD_AHEAD_WIDTHS(6);
	case 7:
		BWD_AHEAD_WIDTHS(7);
	default:
		return 0;
	}
#undef BWD_AHEAD_WIDTHS
}

template <int D, int W>
static void Launch_Backward_Simt(bool b_ahead, const TSimtChunk *chunks, int n_chunks, int n_lds_bytes, const int32_t *prog, const long long *t,
	const double *L, double *w, double *x_out, hipStream_t stream, const TBatch &t_batch)
{
	if constexpr(TBwdAheadDim<D>::b_have) {
		if(b_ahead) {
			hipLaunchKernelGGL((backward_simt_ahead_kernel<D, W, SIMT_BWD_AHEAD>), dim3(n_chunks, t_batch.n), dim3(64), n_lds_bytes, stream,
				chunks, prog, t, L, w, x_out, t_batch);
			return;
		}
	}
	hipLaunchKernelGGL((backward_simt_kernel<D, W>), dim3(n_chunks, t_batch.n), dim3(64), n_lds_bytes, stream, chunks, prog, t, L, w, x_out, t_batch);
}

int backward_simt_ahead_waves(int n_dim, int n_width, int n_lds_bytes)
{
	return simt_resident_workgroups(p_Backward_Ahead_Kernel(n_dim, n_width), 64, n_lds_bytes); // (a workgroup is one wave)
}

// the two-wave form exists where the fetch-ahead form does, for the widths that leave a wave idle lanes or none (16, 32)
static const void *p_Backward_Branches_Kernel(int n_dim, int n_width)
{
	if(n_dim != 6)
		return 0;
	return (n_width == 16)? reinterpret_cast<const void*>(&backward_simt_kernel_branches<6, 16, SIMT_BWD_AHEAD>) :
		(n_width == 32)? reinterpret_cast<const void*>(&backward_simt_kernel_branches<6, 32, SIMT_BWD_AHEAD>) : 0;
}

bool backward_simt_branches_exists(int n_dim, int n_width)
{
	return p_Backward_Branches_Kernel(n_dim, n_width) != 0;
}

int backward_simt_branches_groups(int n_dim, int n_width, int n_lds_bytes)
{
	if(!backward_simt_branches_exists(n_dim, n_width) || n_lds_bytes <= 0)
		return 0;
	return simt_resident_workgroups(p_Backward_Branches_Kernel(n_dim, n_width), 128, n_lds_bytes);
}

bool launch_backward_simt(const TSimtChunk *chunks, int n_chunks, int n_width, int n_lds_bytes, size_t n_lds_limit, int n_ahead_waves, const int32_t *prog, const int64_t *tab,
	int n_dim, const double *L, double *w, double *x_out, hipStream_t stream, const TBatch &t_batch, bool b_report, const TSimtBwdBranchLaunch *p_branches)
{
	if(n_chunks <= 0)
		return true;
	if(n_lds_bytes < 0 || size_t(n_lds_bytes) > n_lds_limit)
		return false; // (the chunk tables are staged in LDS: a launch over the limit would fail without a word)
	const long long *t = reinterpret_cast<const long long*>(tab);
	// The two-wave form (backward_simt_kernel_branches) under the rule of the factor form (launch_factor_simt()): the launch is one
	// the fetch-ahead form would take, fits one round of the two-wave form, has tasks longer than T* columns and is of a stage
	// of at least 2 048 tasks.  Development aid (plan.h): 0 = never, 1 = wherever the stage has records; the same bits.  A launch
	// whose LDS request is over the limit keeps the forms below.
	{
		const int n_branches_env = dev_knob("SLAMPP_HIP_DEV_SIMT_BWD_BRANCHES", -1);
		const int n_ahead_knob = dev_knob("SLAMPP_HIP_DEV_SIMT_BWD_AHEAD", -1);
		const bool b_would_fetch_ahead = p_Backward_Ahead_Kernel(n_dim, n_width) &&
			((n_ahead_knob >= 0)? n_ahead_knob != 0 : int64_t(n_chunks) * std::max<int64_t>(t_batch.n, 1) <= n_ahead_waves);
		const bool b_branches = p_branches && p_branches->n_groups > 0 && backward_simt_branches_exists(n_dim, n_width) &&
			p_branches->n_lds_bytes > 0 && size_t(p_branches->n_lds_bytes) <= n_lds_limit &&
			((n_branches_env >= 0)? n_branches_env != 0 : b_would_fetch_ahead &&
			int64_t(p_branches->n_groups) * std::max<int64_t>(t_batch.n, 1) <= p_branches->n_round_groups &&
			p_branches->n_tstar < p_branches->n_longest_task && p_branches->n_stage_tasks >= 2048);
		if(b_branches) {
			if(b_report)
				fprintf(stderr, "stage_timing lane-per-task backward branches launch: %d workgroups of two waves, %d split chunks, %d whole chunks, width %d, block size %d, %d members\n",
					p_branches->n_groups, p_branches->n_split_chunks, p_branches->n_whole_chunks, n_width, n_dim, int(t_batch.n));
			if(n_width == 16)
				hipLaunchKernelGGL((backward_simt_kernel_branches<6, 16, SIMT_BWD_AHEAD>), dim3(p_branches->n_groups, t_batch.n), dim3(128), p_branches->n_lds_bytes, stream,
					p_branches->groups, prog, t, L, w, x_out, t_batch, p_branches->n_tab_region, p_branches->n_x_region);
			else
				hipLaunchKernelGGL((backward_simt_kernel_branches<6, 32, SIMT_BWD_AHEAD>), dim3(p_branches->n_groups, t_batch.n), dim3(128), p_branches->n_lds_bytes, stream,
					p_branches->groups, prog, t, L, w, x_out, t_batch, p_branches->n_tab_region, p_branches->n_x_region);
			return hipGetLastError() == hipSuccess;
		}
	}
	// The fetch-ahead form runs at one wave a SIMD: it is for launches that fit the chip in one round at that occupancy and so
	// could not hide a wave's waits behind other waves anyway (C3's leaves: 592 waves, 41.7 -> 30.3 us).  Larger
	// launches -- a batch of eight (4 736 waves), a million poses -- keep the kernel above, where many waves a SIMD already hide
	// the waits.  Development aid (plan.h): 0 = never, 1 = wherever the block size has the form; the results are the same bits.
	const int n_ahead_env = dev_knob("SLAMPP_HIP_DEV_SIMT_BWD_AHEAD", -1);
	const void *p_ahead = p_Backward_Ahead_Kernel(n_dim, n_width);
	const bool b_ahead = p_ahead && ((n_ahead_env >= 0)? n_ahead_env != 0 : int64_t(n_chunks) * std::max<int64_t>(t_batch.n, 1) <= n_ahead_waves);
	if(b_report) // (development aid SLAMPP_HIP_STAGE_TIMING: which form the launch takes, for the tests)
		fprintf(stderr, "stage_timing lane-per-task backward launch: %d chunks, width %d, block size %d, %d members, %s\n", n_chunks, n_width, n_dim,
			int(t_batch.n), b_ahead? "fetch ahead" : "fetch by column");
#define BWD_LAUNCH(D_, W_) Launch_Backward_Simt<D_, W_>(b_ahead, chunks, n_chunks, n_lds_bytes, prog, t, L, w, x_out, stream, t_batch)
#define BWD_WIDTHS(D_) do { if(n_width == 16) BWD_LAUNCH(D_, 16); else if(n_width == 32) BWD_LAUNCH(D_, 32); else BWD_LAUNCH(D_, 64); } while(0)
	switch(n_dim) {
	case 3:
		BWD_WIDTHS(3);
		break;
	case 6:
		BWD_WIDTHS(6);
		break;
	case 7:
		BWD_WIDTHS(7);
		break;
	default:
		return false;
	}
#undef BWD_WIDTHS
#undef BWD_LAUNCH
	return hipGetLastError() == hipSuccess;
}

// inv(L_jj) from L_jj, a thread per column (forward substitution on the identity)
template <int D>
__global__ void invert_diagonals_kernel(TDevPlan p, int64_t col_begin, int64_t col_end, const double *__restrict__ L, double *Linv)
{
	const int64_t c = col_begin + int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
	if(c >= col_end)
		return;
	const TColDesc &cd = p.cols[c];
	const double *a = L + p.blks[cd.k0].loff; // element (r, q) at r + q D
	double x[D][D]; // x[r][c]
	#pragma unroll
	for(int q = 0; q < D; ++ q) {
		#pragma unroll
		for(int r = 0; r < D; ++ r) {
			if(r < q)
				x[r][q] = 0.0;
			else {
				double sum = (r == q)? 1.0 : 0.0;
				#pragma unroll
				for(int t = q; t < r; ++ t)
					sum -= a[r + t * D] * x[t][q];
				x[r][q] = sum / a[r + r * D];
			}
		}
	}
	double *p_out = Linv + cd.linv_off;
	#pragma unroll
	for(int q = 0; q < D; ++ q) {
		#pragma unroll
		for(int r = 0; r < D; ++ r)
			p_out[r + q * D] = x[r][q];
	}
}

bool launch_invert_diagonals(const TDevPlan &p, int64_t col_begin, int64_t col_end, const double *L, double *Linv, hipStream_t stream)
{
	if(col_end <= col_begin)
		return true;
	const unsigned n_grid = unsigned((col_end - col_begin + 127) / 128);
	switch(p.uniform_dim) {
	case 3:
		hipLaunchKernelGGL((invert_diagonals_kernel<3>), dim3(n_grid), dim3(128), 0, stream, p, col_begin, col_end, L, Linv);
		return true;
	case 6:
		hipLaunchKernelGGL((invert_diagonals_kernel<6>), dim3(n_grid), dim3(128), 0, stream, p, col_begin, col_end, L, Linv);
		return true;
	case 7:
		hipLaunchKernelGGL((invert_diagonals_kernel<7>), dim3(n_grid), dim3(128), 0, stream, p, col_begin, col_end, L, Linv);
		return true;
	default:
		return false;
	}
}

} // namespace slampp

#include "preload.h"
SLAMPP_PRELOAD_UNIT(simt_kernel) // (the handle's bring-up thread loads this unit's code object: capi.hip)
