// schur.hip -- the BA path: Schur complement of the landmark block, dense reduced camera system,
// back-substitution.  Restates CLinearSolver_Schur::Solve_PosDef_Blocky, steps 2-13
// (/root/reference/include/slam/LinearSolver_Schur.h:1699-1886) for gfx950:
//
//   Lambda = | A U |    S  = A - U C^-1 U^T           (reference: SliceTo / InverseOf_BlockDiag /
//            | V C |    r  = x - U C^-1 l              two MultiplyToWith_FBS / AddTo_FBS / PreMultiply_Add)
//                       dx = S^-1 r                   (reference: Eigen LLT on the densified S)
//                       dl = C^-1 (l - U^T dx)        (reference: PostMultiply_Add + PreMultiply_Add)
//
// Landmarks are independent units (C is block diagonal), so every kernel but the dense factor is a
// stream over the observations: HBM-bound integer/fp64 work, no MFMA.
//   schur_point_inverse : C_p^-1, one thread per point                        (72 B in, 72 B out)
//   schur_obs_W         : W_o = U_o C_p^-1, one thread per observation         (144 B in, 144 B out)
//   schur_gather_S      : one wave per nonzero block of S sums its contributions U_b W_a^T from a
//                         precomputed list -- no atomics, bit-reproducible      (288 B per contribution)
//   schur_rhs           : r_c = x_c - sum W_o l_p, one wave per camera
//   dense_cholesky / dense_backsolve (dense_chol.hip)
//   schur_obs_t, schur_point_backsubst : dl
// Multi-GPU (landmark shards): the all-reduce callback sums [S | r] over the ranks right before the
// dense factorization; only the primary shard adds A and x.
// This file holds the solve path: its kernels, the assembly of the reduced system (schur_assemble_t and the two steps every
// caller of it shares: fill, sum over the ranks), schur_enqueue, the landmarks-only solve, and what the covariance and
// re-solve units (schur_marginals.hip, schur_covariance.hip, schur_resolve.hip) need from these kernels.  The host analysis
// and set-up are in schur_setup.hip, the state and the dispatch on the block sizes in schur_state.h.
#include "schur_state.h"
#include "dense_chol.h"

#include <algorithm>

namespace slampp {

#include "schur_device.inl"

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------

// S(lower) := A^T blocks, r := eta_x   (primary shard only; S was zeroed before).  The reduced system lives either in
// the dense buffer S (leading dimension ld, right-hand side in its last row) or, when p_dst is given, in the packed
// upper block-CSC values of the inner sparse solver (block k of Lambda goes to p_dst[k] as it is) and the vector p_r
template <int DC>
__global__ void schur_scatter_A_kernel(const int64_t *ptr, const int32_t *brow, int64_t nc,
	const double *__restrict__ A, const double *__restrict__ eta, double *S, int ld, int n,
	const int64_t *__restrict__ p_dst, double *p_r)
{
	const int64_t gid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
	const int64_t n_elems = ptr[nc] * DC * DC;
	if(gid < n_elems) {
		const int64_t k = gid / (DC * DC);
		const int e = int(gid - k * (DC * DC)), rr = e % DC, q = e / DC; // element (rr, q) of block k = Lambda(r, c), r <= c
		// column of block k: binary search in ptr[0..nc]
		int64_t lo = 0, hi = nc;
		while(hi - lo > 1) {
			const int64_t mid = (lo + hi) >> 1;
			if(ptr[mid] <= k) lo = mid; else hi = mid;
		}
		const int64_t c = lo, r = brow[k];
		if(p_dst)
			S[p_dst[k] + e] = A[gid]; // the upper block (r, c), as stored
		else
			S[size_t(c * DC + q) + size_t(r * DC + rr) * ld] = A[gid]; // lower block (c, r) = block^T
	}
	if(gid < n) {
		if(p_dst)
			p_r[gid] = eta[gid];
		else
			S[size_t(ld - 1) + size_t(gid) * ld] = eta[gid];
	}
}

template <int DC, int DP>
__global__ void schur_point_inverse_kernel(const int64_t *ptr, int64_t nc, int64_t np, int64_t ubase,
	const double *__restrict__ A, double *Cinv, int *p_flag, const int32_t *__restrict__ p_list = 0)
{
	const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
	if(i >= np)
		return;
	const int64_t pt = p_list? int64_t(p_list[i]) : i; // (np: the length of the list, if there is one)
	const int64_t o1 = ptr[nc + pt + 1] - ptr[nc] - (pt + 1);
	const double *C = A + ubase + o1 * (DC * DP) + pt * (DP * DP);
	double c[DP * DP], inv[DP * DP];
	#pragma unroll
	for(int i = 0; i < DP * DP; ++ i)
		c[i] = C[i];
	if(!spd_inverse<DP>(c, inv))
		atomicOr(p_flag, 1);
	#pragma unroll
	for(int i = 0; i < DP * DP; ++ i)
		Cinv[pt * (DP * DP) + i] = inv[i];
}

template <int DC, int DP>
__global__ void schur_obs_W_kernel(int64_t n_obs, int64_t ubase, const int32_t *obs_pt,
	const double *__restrict__ A, const double *__restrict__ Cinv, double *W, const int32_t *__restrict__ p_list = 0)
{
	const int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
	if(i >= n_obs)
		return;
	const int64_t o = p_list? int64_t(p_list[i]) : i;
	const int64_t pt = obs_pt[o];
	const double *U = A + ubase + o * (DC * DP) + pt * (DP * DP);
	double u[DC * DP], ci[DP * DP];
	#pragma unroll
	for(int i = 0; i < DC * DP; ++ i)
		u[i] = U[i];
	#pragma unroll
	for(int i = 0; i < DP * DP; ++ i)
		ci[i] = Cinv[pt * (DP * DP) + i];
	#pragma unroll
	for(int q = 0; q < DP; ++ q)
		#pragma unroll
		for(int r = 0; r < DC; ++ r) {
			double t = 0;
			#pragma unroll
			for(int k = 0; k < DP; ++ k)
				t += u[r + k * DC] * ci[k + q * DP];
			W[o * (DC * DP) + r + q * DC] = t;
		}
}


// ---- incremental update of the reduced camera system ----
// Stands where the reference's dog-leg solver updates its Schur complement from Omega = Lambda_new - Lambda_old instead
// of recomputing it (include/slam/NonlinearSolver_Lambda_DL.h:1025-1086, 2301-): after a relinearization that moved a
// few landmarks, S_new = S_old + (A_new - A_old) - sum over the changed landmarks of (U C^-1 U^T)_new - (U C^-1 U^T)_old.
// The old contribution of a landmark is rebuilt from what the previous solve left on the device, W = U C^-1 and C^-1
// (U C^-1 U^T = W C W^T), so no copy of the old values is kept; the reduced right-hand side is recomputed in full (eta
// changes everywhere).  Several landmarks may touch one block of S at the same time: fp64 atomic adds, so the sum order --
// unlike everywhere else in this library -- is not fixed (the option is off by default).
template <int DC>
__global__ void schur_delta_A_kernel(const int64_t *ptr, const int32_t *brow, int64_t nc,
	const double *__restrict__ A, double *A_prev, const double *__restrict__ eta, double *S, int ld, int n,
	const int64_t *__restrict__ p_dst, double *p_r)
{
	const int64_t gid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
	const int64_t n_elems = ptr[nc] * DC * DC;
	if(gid < n_elems) {
		const int64_t k = gid / (DC * DC);
		const int e = int(gid - k * (DC * DC)), rr = e % DC, q = e / DC;
		int64_t lo = 0, hi = nc;
		while(hi - lo > 1) {
			const int64_t mid = (lo + hi) >> 1;
			if(ptr[mid] <= k) lo = mid; else hi = mid;
		}
		const int64_t c = lo, r = brow[k];
		const double f_new = A[gid], f_delta = f_new - A_prev[gid];
		A_prev[gid] = f_new;
		if(p_dst)
			S[p_dst[k] + e] += f_delta;
		else
			S[size_t(c * DC + q) + size_t(r * DC + rr) * ld] += f_delta;
	}
	if(gid < n) {
		if(p_dst)
			p_r[gid] = eta[gid];
		else
			S[size_t(ld - 1) + size_t(gid) * ld] = eta[gid];
	}
}

// The contributions of the changed landmarks exchanged, one wave per landmark.  Its observations are taken T = 32 at a
// time: for a tile of "row" observations b the products W_b C (old) and U_b C_new^-1 (the new W_b) go to LDS, then for
// every tile of "column" observations a up to it their U and (old) W blocks; every lane finds the block of S of one
// camera pair (a binary search: a dozen dependent trips to memory), then a lane per (pair, element) adds
// (W_b C W_a^T - U_b C_new^-1 U_a^T)(r, q) to S.  A landmark seen by at most 32 cameras -- nearly all of them -- is one
// tile against itself.  (Until round 3 a landmark with more than 24 observations was walked by the wave's first lane
// alone, k (k + 1) / 2 searches one after the other: 30 such landmarks among 5 000 changed ones of the Venice-like C4
// made the update 6.3 ms, against 1.0 ms for assembling everything again.)
template <int DC, int DP>
__global__ void __launch_bounds__(64)
schur_changed_points_kernel(const int64_t *__restrict__ changed, int64_t n_changed, const int64_t *ptr,
	const int32_t *brow, int64_t nc, int64_t ubase, const double *__restrict__ A, double *Cinv, double *W,
	int64_t n_sblocks, const int32_t *__restrict__ sb_row, const int32_t *__restrict__ sb_col, double *S, int ld,
	const int64_t *__restrict__ p_dst, int *p_flag)
{
	enum { T = 32, BLK = DC * DP, PMAX = T * T };
	__shared__ double s_U[2][T * BLK], s_W[2][T * BLK]; // [0]: the column tile, [1]: the row tile
	__shared__ double s_wc[T * BLK], s_wn[T * BLK];     // of the row tile
	__shared__ int64_t s_dst[PMAX];
	__shared__ int32_t s_cam[2][T];
	const int lane = threadIdx.x;
	const int64_t pt = changed[blockIdx.x];
	const int64_t k0 = ptr[nc + pt], o0 = k0 - ptr[nc] - pt, o1 = ptr[nc + pt + 1] - ptr[nc] - (pt + 1);
	const int k = int(o1 - o0);
	double c_old[DP * DP], ci_old[DP * DP], c_new[DP * DP], ci_new[DP * DP];
	#pragma unroll
	for(int t = 0; t < DP * DP; ++ t) {
		ci_old[t] = Cinv[pt * (DP * DP) + t];
		c_new[t] = A[ubase + o1 * BLK + pt * (DP * DP) + t];
	}
	spd_inverse<DP>(ci_old, c_old); // C of the previous solve
	if(!spd_inverse<DP>(c_new, ci_new) && lane == 0)
		atomicOr(p_flag, 1);
	const int n_tiles = (k + T - 1) / T;
	for(int tb = 0; tb < n_tiles; ++ tb) {
		const int b0 = tb * T, kb = (k - b0 < T)? k - b0 : T;
		__syncthreads(); // (the tile before is done with)
		for(int i = lane; i < kb * BLK; i += 64) { // (a landmark's observations follow one another)
			s_U[1][i] = A[ubase + (o0 + b0) * BLK + pt * (DP * DP) + i];
			s_W[1][i] = W[(o0 + b0) * BLK + i];
		}
		if(lane < kb)
			s_cam[1][lane] = brow[k0 + b0 + lane];
		__syncthreads();
		for(int i = lane; i < kb * BLK; i += 64) { // W_b C_old (old), U_b C^-1_new (the new W_b)
			const int ob = i / BLK, e = i - ob * BLK, r = e % DC, q = e / DC;
			double t_old = 0, t_new = 0;
			#pragma unroll
			for(int t = 0; t < DP; ++ t) {
				t_old += s_W[1][ob * BLK + r + t * DC] * c_old[t + q * DP];
				t_new += s_U[1][ob * BLK + r + t * DC] * ci_new[t + q * DP];
			}
			s_wc[i] = t_old;
			s_wn[i] = t_new;
		}
		for(int ta = 0; ta <= tb; ++ ta) {
			const int a0 = ta * T, ka = (ta == tb)? kb : T;
			const int n_side = (ta == tb)? 1 : 0; // the column tile: the row tile itself on the diagonal
			__syncthreads(); // (s_wc / s_wn are there; the column tile and the destinations before are done with)
			if(ta != tb) {
				for(int i = lane; i < ka * BLK; i += 64) {
					s_U[0][i] = A[ubase + (o0 + a0) * BLK + pt * (DP * DP) + i];
					s_W[0][i] = W[(o0 + a0) * BLK + i];
				}
				if(lane < ka)
					s_cam[0][lane] = brow[k0 + a0 + lane];
				__syncthreads();
			}
			const int n_pairs = (ta == tb)? kb * (kb + 1) / 2 : kb * ka;
			for(int p = lane; p < n_pairs; p += 64) { // pair (b >= a): the block (row cam_b, column cam_a) of S
				int a, b;
				if(ta == tb) { // at b (b + 1) / 2 + a
					b = int((sqrtf(8.0f * float(p) + 1.0f) - 1.0f) * 0.5f);
					while((b + 1) * (b + 2) / 2 <= p) ++ b;
					while(b * (b + 1) / 2 > p) -- b;
					a = p - b * (b + 1) / 2;
				} else {
					b = p / ka;
					a = p - b * ka;
				}
				const int64_t cam_a = s_cam[n_side][a], cam_b = s_cam[1][b];
				if(p_dst) { // binary search on the blocks' sorted keys column * nc + row
					const int64_t key = cam_a * nc + cam_b;
					int64_t lo = 0, hi = n_sblocks - 1;
					while(lo < hi) {
						const int64_t mid = (lo + hi) >> 1;
						if(int64_t(sb_col[mid]) * nc + sb_row[mid] < key) lo = mid + 1; else hi = mid;
					}
					s_dst[p] = p_dst[lo];
				} else
					s_dst[p] = cam_b * DC + cam_a * DC * int64_t(ld);
			}
			__syncthreads();
			for(int i = lane; i < n_pairs * DC * DC; i += 64) {
				const int p = i / (DC * DC), e = i - p * (DC * DC), q = e % DC, r = e / DC; // (q fastest: neighbouring lanes, neighbouring addresses)
				int a, b;
				if(ta == tb) {
					b = int((sqrtf(8.0f * float(p) + 1.0f) - 1.0f) * 0.5f);
					while((b + 1) * (b + 2) / 2 <= p) ++ b;
					while(b * (b + 1) / 2 > p) -- b;
					a = p - b * (b + 1) / 2;
				} else {
					b = p / ka;
					a = p - b * ka;
				}
				double f_old = 0, f_new = 0;
				#pragma unroll
				for(int t = 0; t < DP; ++ t) {
					f_old += s_wc[b * BLK + r + t * DC] * s_W[n_side][a * BLK + q + t * DC]; // (W_b C W_a^T)(r, q)
					f_new += s_wn[b * BLK + r + t * DC] * s_U[n_side][a * BLK + q + t * DC]; // (U_b C^-1 U_a^T)(r, q)
				}
				// S = A - sum U C^-1 U^T: the old term comes back, the new one goes
				const int64_t n_at = p_dst? s_dst[p] + q + r * DC : s_dst[p] + r + q * int64_t(ld);
				atomicAdd(S + n_at, f_old - f_new);
			}
		}
	}
	// every pair of the landmark has read the old W: now it is replaced
	__syncthreads();
	if(n_tiles == 1) {
		for(int i = lane; i < k * BLK; i += 64)
			W[o0 * BLK + i] = s_wn[i];
	} else {
		for(int i = lane; i < k * BLK; i += 64) {
			const int ob = i / BLK, e = i - ob * BLK, r = e % DC, q = e / DC;
			double t_new = 0;
			#pragma unroll
			for(int t = 0; t < DP; ++ t)
				t_new += A[ubase + (o0 + ob) * BLK + pt * (DP * DP) + r + t * DC] * ci_new[t + q * DP];
			W[o0 * BLK + i] = t_new;
		}
	}
	if(lane < DP * DP)
		Cinv[pt * (DP * DP) + lane] = ci_new[lane];
}

// one workgroup of W waves per nonzero block of S: S(row, col) -= sum_e U_b W_a^T; contribution e is
// summed by wave e mod W, the partial sums are combined in a fixed order (bit-reproducible).
// The kernel is bound by the address path, not by bytes, so it spends as few vector-memory
// instructions as it can: the entry indices are fetched 64 at a time (one coalesced load, then
// v_readlane), the two operand blocks of an entry with ONE load (lanes 0..17 U_b, lanes 18..35 W_a,
// both contiguous) into LDS, eight entries per batch; a batch is then one small GEMM on the matrix cores
// (v_mfma_f64_16x16x4: S block += [U_1 .. U_8] [W_1 .. W_8]^T, K = 24).  All eight requests of a batch are issued
// before the first LDS store: written as "load, store" per entry the compiler serialized them, eight memory
// latencies per batch (0.71 -> 0.50 ms at C4 once hoisted).  Measured and not kept: batches of 16 (slower), an
// XCD-contiguous block order, camera-major copies of U and W (gather 4 % faster, the scattered writes of the copy
// cost 0.24 ms).  144-byte operand blocks straddle 64-byte sectors: about 1.9x the algorithmic bytes are fetched.
template <int DC, int DP, int W>
__global__ void __launch_bounds__(64 * W)
schur_gather_S_kernel(int64_t n_sblocks, const int64_t *sb_ptr, const int32_t *sb_row, const int32_t *sb_col,
	const int32_t *ent_a, const int64_t *ent_uoff, const double *__restrict__ A, const double *__restrict__ W_,
	double *S, int ld, const int64_t *__restrict__ p_dst, const int32_t *__restrict__ sb_map)
{
	enum { BLK = DC * DP, BATCH = 8 };
	__shared__ double s_ops[W][BATCH][2 * BLK];
	__shared__ double s_part[W][64];
	const int64_t n_list = blockIdx.x; // list n_list serves block sb of S (the same, unless only some landmarks go through lists)
	const int64_t sb = sb_map? int64_t(sb_map[n_list]) : n_list;
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const bool b_act = lane < DC * DC;
	const int r = b_act? lane % DC : 0, q = b_act? lane / DC : 0;
	// Every lane loads (lanes past the two operand blocks repeat the last element: same cache line, no branch around
	// the load): lanes 0 .. BLK-1 the block U_b at A + u, the others W_a at W_ + a BLK.  All of this is there to keep the
	// wave-instruction count of an entry down -- with eight waves per SIMD
	// resident the kernel is bound by instruction issue around its loads, not by the loads.
	const int lane_c = (lane < 2 * BLK)? lane : 2 * BLK - 1;
	const bool b_u = lane_c < BLK;
	const int64_t lane_off = b_u? lane_c : lane_c - BLK;
	typedef double v4f64 __attribute__((ext_vector_type(4)));
	v4f64 macc = {0, 0, 0, 0};
	// the MFMA fragment a lane reads for step q4 of a batch: entry, and offset of its element of U inside s_ops[wave]
	int frag_ent[BATCH * DP / 4], frag_off[BATCH * DP / 4];
	#pragma unroll
	for(int q4 = 0; q4 < BATCH * DP / 4; ++ q4) {
		const int kg = 4 * q4 + (lane >> 4), ent = kg / DP, t = kg % DP;
		const int m = lane & 15, mm = (m < DC)? m : 0;
		frag_ent[q4] = ent;
		frag_off[q4] = ent * (2 * BLK) + mm + t * DC;
	}
	const double *s_my = &s_ops[wave][0][0];
	const int64_t e0 = sb_ptr[n_list], e1 = sb_ptr[n_list + 1];
	// this wave's entries: e0 + wave, e0 + wave + W, ...; processed in chunks of 64
	for(int64_t base = e0 + wave; base < e1; base += int64_t(64) * W) {
		const int64_t my = base + int64_t(lane) * W;
		const int32_t my_a = (my < e1)? ent_a[my] : 0;
		const int64_t my_u = (my < e1)? ent_uoff[my] : 0;
		const int n_chunk = int(min(int64_t(64), (e1 - base + W - 1) / W));
		for(int i = 0; i < n_chunk; i += BATCH) {
			double v[BATCH]; // all requests of the batch first, then the LDS stores: one memory latency per batch, not eight
			#pragma unroll
			for(int j = 0; j < BATCH; ++ j) {
				const int idx = min(i + j, n_chunk - 1); // the tail re-reads the last entry, its product is skipped below
				const int32_t a = __builtin_amdgcn_readlane(my_a, idx);
				const int64_t u = (int64_t(__builtin_amdgcn_readlane(int(my_u >> 32), idx)) << 32) |
					uint32_t(__builtin_amdgcn_readlane(int(my_u), idx));
				const double *p_src = b_u? A + u : W_ + int64_t(a) * BLK; // two arrays, one load: the lane picks its base
				v[j] = p_src[lane_off];
			}
			if(lane < 2 * BLK) {
				#pragma unroll
				for(int j = 0; j < BATCH; ++ j)
					s_ops[wave][j][lane] = v[j];
			}
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
			// the batch is one small GEMM: S block (DC x DC) += [U_1 .. U_BATCH] [W_1 .. W_BATCH]^T with K = BATCH * DP,
			// four k at a time on the matrix cores (rows / columns >= DC of the 16 x 16 tile are don't-cares)
			const int n_left = n_chunk - i; // entries of the batch that exist
			#pragma unroll
			for(int q4 = 0; q4 < BATCH * DP / 4; ++ q4) {
				const double a = (frag_ent[q4] < n_left)? s_my[frag_off[q4]] : 0.0; // the tail repeats its last entry: not summed
				const double b = s_my[frag_off[q4] + BLK];
				macc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, macc, 0, 0, 0);
			}
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
			__builtin_amdgcn_wave_barrier();
			__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
		}
	}
	// lane l holds the tile elements ((l >> 4) + 4 reg, l & 15): hand the DC x DC corner to the lanes that write it
	#pragma unroll
	for(int reg = 0; reg < 4; ++ reg) {
		const int row = (lane >> 4) + 4 * reg, col = lane & 15;
		if(row < DC && col < DC)
			s_part[wave][row + col * DC] = macc[reg];
	}
	__syncthreads();
	if(wave != 0)
		return;
	double acc = 0;
	if(b_act) {
		#pragma unroll
		for(int ww = 0; ww < W; ++ ww)
			acc += s_part[ww][lane];
	}
	if(b_act) { // dense: the lower block (row, col); packed: its transpose, the upper block (col, row) of the inner solver
		const size_t idx = p_dst? size_t(p_dst[sb]) + q + r * DC :
			size_t(int64_t(sb_row[sb]) * DC + r) + size_t(int64_t(sb_col[sb]) * DC + q) * ld;
		S[idx] -= acc;
	}
}

// one wave per camera: r_c -= sum over its observations of W_o l_p
template <int DC, int DP>
__global__ void __launch_bounds__(64)
schur_rhs_kernel(const int64_t *cam_ptr, const int32_t *cam_obs, const int32_t *obs_pt, int n,
	const double *__restrict__ W, const double *__restrict__ eta, double *S, int ld, double *p_r)
{
	const int64_t c = blockIdx.x;
	const int lane = threadIdx.x;
	double acc[DC];
	#pragma unroll
	for(int i = 0; i < DC; ++ i)
		acc[i] = 0;
	const int64_t e1 = cam_ptr[c + 1];
	for(int64_t e = cam_ptr[c] + lane; e < e1; e += 64) {
		const int64_t o = cam_obs[e];
		const double *Wo = W + o * (DC * DP), *l = eta + n + int64_t(obs_pt[o]) * DP;
		#pragma unroll
		for(int t = 0; t < DP; ++ t) {
			const double lt = l[t];
			#pragma unroll
			for(int i = 0; i < DC; ++ i)
				acc[i] += Wo[i + t * DC] * lt;
		}
	}
	#pragma unroll
	for(int i = 0; i < DC; ++ i) {
		#pragma unroll
		for(int m = 32; m >= 1; m >>= 1)
			acc[i] += __shfl_xor(acc[i], m);
	}
	if(lane == 0) {
		#pragma unroll
		for(int i = 0; i < DC; ++ i) {
			if(p_r)
				p_r[c * DC + i] -= acc[i];
			else
				S[size_t(ld - 1) + size_t(c * DC + i) * ld] -= acc[i];
		}
	}
}

// T_o = U_o^T dx_cam(o), one lane per observation.  The U blocks of 64 consecutive observations are one contiguous piece of
// the values (with the C blocks of the landmarks they belong to in between): the wave fetches that piece with coalesced
// loads into LDS and every lane reads its block from there -- a lane fetching its own 144 bytes touched 64 lines per
// load instruction (94 us at C4 for 288 MB; the back-substitution was a third of a C5-size step)
template <int DC, int DP>
__global__ void __launch_bounds__(64)
schur_obs_t_kernel(int64_t n_obs, int64_t ubase, int64_t nc, const int64_t *ptr, const int32_t *brow,
	const int32_t *obs_pt, const double *__restrict__ A, const double *__restrict__ dx, double *T)
{
	enum { BLK = DC * DP, PIECE = 64 * BLK + 24 * DP * DP, // room for 24 C blocks in between (64 observations of landmarks with three or more each)
		N_LOADS = (PIECE + 2 + 127) / 128 }; // 16-byte requests per lane that bring a whole piece (one double of slack at either end)
	typedef double v2f64 __attribute__((ext_vector_type(2)));
	__shared__ __attribute__((aligned(16))) double s_u[N_LOADS * 128];
	const int lane = threadIdx.x;
	const int64_t o_first = int64_t(blockIdx.x) * 64;
	const int64_t o = min(o_first + lane, n_obs - 1); // (the tail repeats the last observation)
	const int64_t pt = obs_pt[o];
	const int64_t n_off = o * BLK + pt * (DP * DP); // offset of U_o behind ubase
	const int64_t n_off_first = (int64_t(__builtin_amdgcn_readlane(int(n_off >> 32), 0)) << 32) | uint32_t(__builtin_amdgcn_readlane(int(n_off), 0));
	const int64_t n_off_last = (int64_t(__builtin_amdgcn_readlane(int(n_off >> 32), 63)) << 32) | uint32_t(__builtin_amdgcn_readlane(int(n_off), 63));
	const int64_t n_piece = n_off_last - n_off_first + BLK;
	const bool b_staged = n_piece <= PIECE && (reinterpret_cast<uintptr_t>(A) & 15) == 0; // (wave-uniform; many one- or two-camera landmarks in a row:
	// every lane fetches its own block -- and so where the caller's values start at an odd double: the 16-byte requests below
	// count on an even one; slampp_hip_factor_solve_device_async passes the caller's pointer through unchecked: advisor, round 5)
	// (round 5) the whole piece is requested at once, in 16-byte pieces -- up to eleven per lane in flight -- and the camera's dx
	// beside it: the loop of eight 8-byte requests, wait, store took up to three round trips a wave, and the gather of dx a
	// fourth behind them.  A landmark's blocks start at an odd double where an odd number of 3 x 3 blocks precedes them: the
	// piece is fetched from the even double at or before its first one (n_shift), which stays inside the values.
	const int n_shift = int((ubase + n_off_first) & 1);
	const int n_piece_al = (int(n_piece) + n_shift + 1) & ~1; // doubles fetched: from the even double before the piece to the one after it
	v2f64 v[N_LOADS];
	if(b_staged) {
		const double *p_src = A + (ubase + n_off_first - n_shift);
		#pragma unroll
		for(int u = 0; u < N_LOADS; ++ u) {
			const int e = 2 * (64 * u + lane);
			v[u] = *reinterpret_cast<const v2f64*>(p_src + ((e < n_piece_al)? e : 0)); // (past the end: the first pair again)
		}
	}
	const int64_t cam = brow[ptr[nc] + o + pt]; // block index of observation o = ptr[nc] + o + (number of C blocks before it)
	double x[DC];
	#pragma unroll
	for(int i = 0; i < DC; ++ i)
		x[i] = dx[cam * DC + i];
	if(b_staged) {
		#pragma unroll
		for(int u = 0; u < N_LOADS; ++ u) {
			const int e = 2 * (64 * u + lane);
			if(e < n_piece_al)
				*reinterpret_cast<v2f64*>(s_u + e) = v[u];
		}
	}
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
	const double *U = b_staged? s_u + (n_off - n_off_first) + n_shift : A + ubase + n_off;
	if(o_first + lane < n_obs) {
		#pragma unroll
		for(int t = 0; t < DP; ++ t) {
			double sum = 0;
			#pragma unroll
			for(int i = 0; i < DC; ++ i)
				sum += U[i + t * DC] * x[i];
			T[o * DP + t] = sum;
		}
	}
}

template <int DC, int DP>
__global__ void schur_point_backsubst_kernel(const int64_t *ptr, int64_t nc, int64_t np, int n,
	const double *__restrict__ Cinv, const double *__restrict__ T, const double *__restrict__ dx, double *out)
{
	const int64_t gid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
	if(gid < np) {
		const int64_t pt = gid;
		const int64_t o0 = ptr[nc + pt] - ptr[nc] - pt, o1 = ptr[nc + pt + 1] - ptr[nc] - (pt + 1);
		double v[DP];
		#pragma unroll
		for(int t = 0; t < DP; ++ t)
			v[t] = out[n + pt * DP + t];
		for(int64_t o = o0; o < o1; ++ o) {
			#pragma unroll
			for(int t = 0; t < DP; ++ t)
				v[t] -= T[o * DP + t];
		}
		#pragma unroll
		for(int r = 0; r < DP; ++ r) {
			double s = 0;
			#pragma unroll
			for(int t = 0; t < DP; ++ t)
				s += Cinv[pt * (DP * DP) + r + t * DP] * v[t];
			out[n + pt * DP + r] = s;
		}
	}
	if(gid < n)
		out[gid] = dx[gid];
}

// multi-GPU exchange: copies the union blocks of S (and the right-hand side row) into / out of one contiguous buffer
__global__ void __launch_bounds__(64)
schur_pack_kernel(const int32_t *__restrict__ un_row, const int32_t *__restrict__ un_col, int64_t n_union, int dc,
	double *S, int ld, int n, double *pack, int b_unpack)
{
	const int64_t b = blockIdx.x;
	const int lane = threadIdx.x;
	double *p_s, *p_p;
	if(b < n_union) {
		if(lane >= dc * dc)
			return;
		p_s = S + size_t(un_row[b] * dc + lane % dc) + size_t(un_col[b] * dc + lane / dc) * ld;
		p_p = pack + b * dc * dc + lane;
	} else {
		const int64_t i = (b - n_union) * 64 + lane;
		if(i >= n)
			return;
		p_s = S + size_t(ld - 1) + size_t(i) * ld;
		p_p = pack + n_union * dc * dc + i;
	}
	if(b_unpack)
		*p_s = *p_p;
	else
		*p_p = *p_s;
}

// Landmark shards: a rank whose own landmarks gave a C_p that is not positive definite must not be the only one to
// return false (the others would carry on into the next collective without it).  The status travels with the data:
// that rank poisons the first entry of its partial reduced right-hand side before the exchange, and every rank looks
// at the sum afterwards.
__global__ void schur_flag_poison_kernel(const int *p_flag, double *p_rhs0)
{
	if(*p_flag)
		*p_rhs0 = __builtin_nan("");
}

__global__ void schur_flag_check_kernel(const double *p_rhs0, int *p_flag)
{
	const double f = *p_rhs0;
	if(f != f)
		atomicOr(p_flag, 1);
}

// S -= U C^-1 U^T and r -= U C^-1 l for all landmarks, C^-1 (and W = U C^-1 for all observations, if b_store_W) left
// behind: S is the dense buffer (ld) or, with p_sb_dst, the packed values of the inner solver (p_r its right-hand side)
template <int DC, int DP>
static void schur_assemble_t(slampp_hip_solver &s, CSchurState &S, const double *A, const double *rhs, double *p_S, int ld,
	const int64_t *p_sb_dst, double *p_r, bool b_store_W)
{
	hipStream_t st = s.stream;
	const int n = S.N;
	const int64_t ubase = S.n_ablocks * DC * DC;
	// Landmarks go through the tiles of schur_tiles.hip (read once each), through the contribution lists, or -- when only
	// some of them fit the tiles -- both: the tiles take theirs, the lists the rest.
	const CSchurTiles &T = S.tiles;
	const bool b_tiles = T.b_enabled, b_lists_all = !b_tiles;
	// (a phase that launches nothing records no events: an event pair costs microseconds of stream time)
	if(b_lists_all || T.b_hybrid)
		s.Phase_Begin("schur_points");
	if(b_lists_all) {
		hipLaunchKernelGGL((schur_point_inverse_kernel<DC, DP>), dim3(unsigned((S.np + 255) / 256)), dim3(256), 0, st,
			S.d_ptr.p(), S.nc, S.np, ubase, A, S.d_Cinv.p(), s.d_flag.p(), (const int32_t*)0);
		hipLaunchKernelGGL((schur_obs_W_kernel<DC, DP>), dim3(unsigned((S.n_obs + 255) / 256)), dim3(256), 0, st,
			S.n_obs, ubase, S.d_obs_pt.p(), A, S.d_Cinv.p(), S.d_W.p(), (const int32_t*)0);
	} else if(T.b_hybrid) { // only the landmarks of the lists: the others get C^-1 (and W) where they are multiplied
		hipLaunchKernelGGL((schur_point_inverse_kernel<DC, DP>), dim3(unsigned((T.n_list_points + 255) / 256)), dim3(256), 0, st,
			S.d_ptr.p(), S.nc, T.n_list_points, ubase, A, S.d_Cinv.p(), s.d_flag.p(), T.d_xpoints.p());
		if(T.n_xobs)
			hipLaunchKernelGGL((schur_obs_W_kernel<DC, DP>), dim3(unsigned((T.n_xobs + 255) / 256)), dim3(256), 0, st,
				T.n_xobs, ubase, S.d_obs_pt.p(), A, S.d_Cinv.p(), S.d_W.p(), T.d_xcam_obs.p());
	}
	if(b_lists_all || T.b_hybrid)
		s.Phase_End();

	if(b_tiles) {
		s.Phase_Begin("schur_tiles");
		// (C^-1 of every landmark is needed by the back-substitution; W only if the next solve may be an update)
		schur_tiles_enqueue(T, DC, DP, S.d_ptr.p(), S.nc, ubase, A, rhs, n, S.d_Cinv.p(), b_store_W? S.d_W.p() : 0,
			true, S.d_sb_row.p(), S.d_sb_col.p(), p_S, ld, p_sb_dst, p_r, s.d_flag.p(), st);
		s.Phase_End();
	}

	if((b_lists_all? S.n_sblocks : T.n_xblocks) > 0) {
		s.Phase_Begin("schur_gather");
		const int64_t n_lists = b_lists_all? S.n_sblocks : T.n_xblocks, n_list_entries = b_lists_all? S.n_entries : T.n_xentries;
		const int64_t *p_list_ptr = b_lists_all? S.d_sb_ptr.p() : T.d_xsb_ptr.p();
		const int32_t *p_list_a = b_lists_all? S.d_ent_a.p() : T.d_xent_a.p(), *p_list_map = b_lists_all? 0 : T.d_xsb_map.p();
		const int64_t *p_list_uoff = b_lists_all? S.d_ent_uoff.p() : T.d_xent_uoff.p();
		if(n_lists > 0) {
			// one wave per block of S for short contribution lists (dense S: 500k blocks x 10 contributions),
			// 8 waves per block for long ones (C4's band structure: 4000 blocks x 1250 contributions: 1.18 -> 0.69 ms)
			if(n_list_entries > 256 * n_lists)
				hipLaunchKernelGGL((schur_gather_S_kernel<DC, DP, 8>), dim3(unsigned(n_lists)), dim3(512), 0, st,
					n_lists, p_list_ptr, S.d_sb_row.p(), S.d_sb_col.p(), p_list_a, p_list_uoff, A,
					S.d_W.p(), p_S, ld, p_sb_dst, p_list_map);
			else
				hipLaunchKernelGGL((schur_gather_S_kernel<DC, DP, 1>), dim3(unsigned(n_lists)), dim3(64), 0, st,
					n_lists, p_list_ptr, S.d_sb_row.p(), S.d_sb_col.p(), p_list_a, p_list_uoff, A,
					S.d_W.p(), p_S, ld, p_sb_dst, p_list_map);
		}
		s.Phase_End();
	}

	if(!S.tiles.b_enabled || S.tiles.b_hybrid) { // (the tiles bring the right-hand side's share of their landmarks themselves)
		s.Phase_Begin("schur_rhs");
		if(!S.tiles.b_enabled)
			hipLaunchKernelGGL((schur_rhs_kernel<DC, DP>), dim3(unsigned(S.nc)), dim3(64), 0, st,
				S.d_cam_ptr.p(), S.d_cam_obs.p(), S.d_obs_pt.p(), n, S.d_W.p(), rhs, p_S, ld, p_r);
		else
			hipLaunchKernelGGL((schur_rhs_kernel<DC, DP>), dim3(unsigned(S.nc)), dim3(64), 0, st,
				S.tiles.d_xcam_ptr.p(), S.tiles.d_xcam_obs.p(), S.d_obs_pt.p(), n, S.d_W.p(), rhs, p_S, ld, p_r);
		s.Phase_End();
	}
}

// The reduced system filled from these values: the destination zeroed -- the dense buffer p_S (padding prepared) or, with
// b_sparse, the inner solver's packed values and the right-hand side behind them --, A and the camera part of rhs scattered in
// on the primary shard, then every landmark's contribution (schur_assemble_t).  The zeroing and the scatter are the phase
// p_s_phase, which in_phase() may add to before it ends.
template <int DC, int DP, class F>
static void schur_fill_t(slampp_hip_solver &s, CSchurState &S, const double *A, const double *rhs, double *p_S, bool b_sparse,
	bool b_store_W, const char *p_s_phase, F in_phase)
{
	hipStream_t st = s.stream;
	const int ld = S.Npad, n = S.N;
	const size_t n_in_values = size_t(S.n_in_blocks) * DC * DC;
	double *p_r = b_sparse? p_S + n_in_values : 0;
	s.Phase_Begin(p_s_phase);
	if(b_sparse)
		SLAMPP_HIP_CHECK(hipMemsetAsync(p_S, 0, (n_in_values + size_t(n)) * sizeof(double), st));
	else {
		SLAMPP_HIP_CHECK(hipMemsetAsync(p_S, 0, size_t(ld) * ld * sizeof(double), st));
		dense_prepare_padding(p_S, ld, n, st);
	}
	if(s.b_shard_primary) {
		const int64_t n_work = std::max<int64_t>(S.n_ablocks * DC * DC, n);
		hipLaunchKernelGGL((schur_scatter_A_kernel<DC>), dim3(unsigned((n_work + 255) / 256)), dim3(256), 0, st,
			S.d_ptr.p(), S.d_brow.p(), S.nc, A, rhs, p_S, ld, n, b_sparse? S.d_a_dst.p() : (const int64_t*)0, p_r);
	}
	in_phase();
	s.Phase_End();
	schur_assemble_t<DC, DP>(s, S, A, rhs, p_S, ld, b_sparse? S.d_sb_dst.p() : (const int64_t*)0, p_r, b_store_W);
}

// The reduced system summed over the ranks (the caller has an all-reduce callback).  Landmark shards: a rank whose own
// landmarks gave a C_p that is not positive definite poisons its partial right-hand side before the exchange and every
// rank looks at the sum afterwards (schur_flag_poison_kernel).  The packed values and the right-hand side of the sparse
// reduced system are one buffer, and every rank built it from the same block list; of the dense buffer, the blocks the
// ranks agreed on travel packed if b_may_pack, else -- and where there are too many cameras to agree on a list -- the
// whole buffer is summed (only the lower triangle and the rhs row carry data).
template <int DC, int DP>
static void schur_sum_over_ranks_t(slampp_hip_solver &s, CSchurState &S, double *p_S, bool b_sparse, bool b_may_pack)
{
	hipStream_t st = s.stream;
	const int ld = S.Npad, n = S.N;
	const size_t n_in_values = size_t(S.n_in_blocks) * DC * DC;
	double *p_rhs0 = b_sparse? p_S + n_in_values : p_S + n; // dense: the right-hand side is row n of S
	s.Phase_Begin("allreduce");
	hipLaunchKernelGGL(schur_flag_poison_kernel, dim3(1), dim3(1), 0, st, s.d_flag.p(), p_rhs0);
	if(b_sparse) {
		if(s.p_allreduce(s.p_allreduce_context, p_S, n_in_values + size_t(n), (void*)st) != 0)
			throw CDeviceError("all-reduce callback failed");
	} else if(S.b_union_dense || !b_may_pack) {
		if(s.p_allreduce(s.p_allreduce_context, p_S, size_t(ld) * ld, (void*)st) != 0)
			throw CDeviceError("all-reduce callback failed");
	} else {
		const unsigned n_grid = unsigned(S.n_union + (n + 63) / 64);
		const size_t n_count = size_t(S.n_union) * DC * DC + size_t(n);
		hipLaunchKernelGGL(schur_pack_kernel, dim3(n_grid), dim3(64), 0, st, S.d_un_row.p(), S.d_un_col.p(), S.n_union, DC,
			p_S, ld, n, S.d_pack.p(), 0);
		if(s.p_allreduce(s.p_allreduce_context, S.d_pack.p(), n_count, (void*)st) != 0)
			throw CDeviceError("all-reduce callback failed");
		hipLaunchKernelGGL(schur_pack_kernel, dim3(n_grid), dim3(64), 0, st, S.d_un_row.p(), S.d_un_col.p(), S.n_union, DC,
			p_S, ld, n, S.d_pack.p(), 1);
	}
	hipLaunchKernelGGL(schur_flag_check_kernel, dim3(1), dim3(1), 0, st, p_rhs0, s.d_flag.p());
	s.Phase_End();
}

template <int DC, int DP>
static void schur_enqueue_t(slampp_hip_solver &s, CSchurState &S, const double *A, double *rhs)
{
	hipStream_t st = s.stream;
	const int ld = S.Npad, n = S.N;
	const int64_t ubase = S.n_ablocks * DC * DC;
	// first step (or a new all-reduce callback): the ranks agree on the blocks of S, then it is decided whether the
	// reduced system is assembled into the dense buffer or straight into the inner sparse solver's values
	if(s.p_allreduce && (S.p_union_fn != s.p_allreduce || S.p_union_context != s.p_allreduce_context))
		schur_agree_on_union(s, S);
	if(!S.b_reduced_decided)
		schur_setup_reduced(s, S);
	const bool b_sparse = S.b_reduced_sparse;
	const size_t n_in_values = size_t(S.n_in_blocks) * DC * DC;
	// option "schur_incremental": what this solve assembles is kept (the dense system in a buffer of its own: the
	// factorization works in place), and a solve that names the changed landmarks updates it instead of rebuilding it
	const bool b_keep = s.n_schur_incremental != 0 && !s.p_allreduce && s.b_shard_primary;
	// option "schur_keep": W is stored as well, so that slampp_hip_solve_again can substitute with what this solve leaves
	const bool b_store_W = b_keep || schur_keeps_for_resolve(s);
	// ... when that is the shorter way (option value 1; 2 = whenever a list is given): the update exchanges the listed
	// landmarks' contributions with atomic adds (C4: 0.44 ms a solve at 500 landmarks, 0.46 at 5 000, 0.51 at 15 000, 0.69
	// at 50 000) and rebuilds the reduced right-hand side; the landmark-major assembly rebuilds everything (0.55 ms a
	// solve), the contribution lists take a millisecond longer (there the update still wins at 50 000: 4.6 against 5.5 ms)
	const bool b_pays = s.n_schur_incremental >= 2 || S.n_changed * (S.tiles.b_enabled? 32 : 4) <= S.np;
	const bool b_update = b_keep && S.b_prev_valid && S.n_changed >= 0 && b_pays;
	if(b_keep) {
		S.d_A_prev.Alloc(size_t(S.n_ablocks) * DC * DC);
		if(!b_sparse)
			S.d_S_unf.Alloc(size_t(ld) * ld);
	}
	double *p_S = b_sparse? S.d_in_buf.p() : ((b_keep)? S.d_S_unf.p() : S.d_S.p()); // where the blocks go
	double *p_r = b_sparse? S.d_in_buf.p() + n_in_values : 0;   // the reduced right-hand side, if it is a vector of its own
	const int64_t *p_sb_dst = b_sparse? S.d_sb_dst.p() : 0, *p_a_dst = b_sparse? S.d_a_dst.p() : 0;

	if(b_update) {
		s.Phase_Begin("schur_update");
		const int64_t n_work = std::max<int64_t>(S.n_ablocks * DC * DC, n);
		hipLaunchKernelGGL((schur_delta_A_kernel<DC>), dim3(unsigned((n_work + 255) / 256)), dim3(256), 0, st,
			S.d_ptr.p(), S.d_brow.p(), S.nc, A, S.d_A_prev.p(), rhs, p_S, ld, n, p_a_dst, p_r);
		if(S.n_changed > 0)
			hipLaunchKernelGGL((schur_changed_points_kernel<DC, DP>), dim3(unsigned(S.n_changed)), dim3(64), 0, st,
				S.d_changed.p(), S.n_changed, S.d_ptr.p(), S.d_brow.p(), S.nc, ubase, A, S.d_Cinv.p(), S.d_W.p(), S.n_sblocks,
				S.d_sb_row.p(), S.d_sb_col.p(), p_S, ld, p_sb_dst, s.d_flag.p());
		s.Phase_End();
	} else {
		schur_fill_t<DC, DP>(s, S, A, rhs, p_S, b_sparse, b_store_W, "schur_init", [&]() {
			if(b_keep)
				SLAMPP_HIP_CHECK(hipMemcpyAsync(S.d_A_prev.p(), A, size_t(S.n_ablocks) * DC * DC * sizeof(double), hipMemcpyDeviceToDevice, st));
		});
	}
	S.b_prev_valid = b_keep; // (a solve that turns out not positive definite takes it back: slampp_hip_sync)
	S.n_changed = -1;        // the list serves one solve

	if(b_update) { // (a full assembly brings the reduced right-hand side itself)
		s.Phase_Begin("schur_rhs");
		hipLaunchKernelGGL((schur_rhs_kernel<DC, DP>), dim3(unsigned(S.nc)), dim3(64), 0, st,
			S.d_cam_ptr.p(), S.d_cam_obs.p(), S.d_obs_pt.p(), n, S.d_W.p(), rhs, p_S, ld, p_r);
		s.Phase_End();
	}

	// option "schur_distributed" (members of a device group, dense reduced system): reduce-scatter + joint factorization
	const bool b_distributed = s.p_allreduce && !b_sparse && s.n_schur_distributed != 0 && s.p_dense_factor != 0;
	if(b_distributed) {
		s.Phase_Begin("dense_chol_distributed");
		if(s.p_dense_factor(s.p_dense_factor_context, p_S, ld, n, S.d_invdiag.p(), s.d_flag.p(), (void*)st) != 0)
			throw CDeviceError("distributed factorization of the reduced camera system failed");
		s.Phase_End();
	} else if(s.p_allreduce)
		schur_sum_over_ranks_t<DC, DP>(s, S, p_S, b_sparse, true);

	const double *p_dx;
	if(b_sparse) {
		s.Phase_Begin("reduced_sparse");
		S.p_inner->p_flag_shared = s.d_flag.p();
		S.p_inner->n_panel_rows = s.n_panel_rows; // (read at every launch)
		S.p_inner->n_panel_backward = s.n_panel_backward;
		S.p_inner->Enqueue_Sparse(p_S, p_r, true); // p_r: the reduced right-hand side on entry, dx on return
		s.Phase_End();
		p_dx = p_r;
	} else {
		if(!b_distributed) {
			s.Phase_Begin("dense_chol");
			if(b_keep) { // the assembled system stays as it is; its copy is factored
				SLAMPP_HIP_CHECK(hipMemcpyAsync(S.d_S.p(), p_S, size_t(ld) * ld * sizeof(double), hipMemcpyDeviceToDevice, st));
				p_S = S.d_S.p();
			}
			dense_cholesky(p_S, ld, n, S.d_invdiag.p(), s.d_flag.p(), st);
			s.Phase_End();
		}
		s.Phase_Begin("dense_solve");
		dense_backsolve(p_S, ld, n, S.d_invdiag.p(), S.d_z.p(), S.d_x.p(), st);
		s.Phase_End();
		p_dx = S.d_x.p();
	}

	s.Phase_Begin("backsubst");
	hipLaunchKernelGGL((schur_obs_t_kernel<DC, DP>), dim3(unsigned((S.n_obs + 63) / 64)), dim3(64), 0, st,
		S.n_obs, ubase, S.nc, S.d_ptr.p(), S.d_brow.p(), S.d_obs_pt.p(), A, p_dx, S.d_t.p());
	const int64_t n_work = std::max<int64_t>(S.np, n);
	hipLaunchKernelGGL((schur_point_backsubst_kernel<DC, DP>), dim3(unsigned((n_work + 255) / 256)), dim3(256), 0, st,
		S.d_ptr.p(), S.nc, S.np, n, S.d_Cinv.p(), S.d_t.p(), p_dx, rhs);
	s.Phase_End();
	SLAMPP_HIP_CHECK(hipGetLastError());
}

// dl_p = C_p^-1 l_p, dx = 0
template <int DP>
__global__ void schur_landmarks_only_kernel(int64_t np, int n, const double *__restrict__ Cinv, double *out)
{
	const int64_t gid = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
	if(gid < np) {
		double v[DP];
		#pragma unroll
		for(int t = 0; t < DP; ++ t)
			v[t] = out[n + gid * DP + t];
		#pragma unroll
		for(int r = 0; r < DP; ++ r) {
			double sum = 0;
			#pragma unroll
			for(int t = 0; t < DP; ++ t)
				sum += Cinv[gid * (DP * DP) + r + t * DP] * v[t];
			out[n + gid * DP + r] = sum;
		}
	}
	if(gid < n)
		out[gid] = 0.0;
}

template <int DC, int DP>
static void schur_enqueue_marginal_t(slampp_hip_solver &s, CSchurState &S, const double *A, double *rhs)
{
	hipStream_t st = s.stream;
	const int64_t ubase = S.n_ablocks * DC * DC;
	s.Phase_Begin("landmarks_only");
	hipLaunchKernelGGL((schur_point_inverse_kernel<DC, DP>), dim3(unsigned((S.np + 255) / 256)), dim3(256), 0, st,
		S.d_ptr.p(), S.nc, S.np, ubase, A, S.d_Cinv.p(), s.d_flag.p());
	const int64_t n_work = std::max<int64_t>(S.np, S.N);
	hipLaunchKernelGGL((schur_landmarks_only_kernel<DP>), dim3(unsigned((n_work + 255) / 256)), dim3(256), 0, st,
		S.np, S.N, S.d_Cinv.p(), rhs);
	s.Phase_End();
	SLAMPP_HIP_CHECK(hipGetLastError());
}

// the covariances when the reduced system is factored by the sparse block path: the same assembly as a solve (into the
// inner solver's packed values, summed over the ranks), its factorization -- the blocks of S^-1 then come on the factor's
// pattern (sparse_inverse.hip) instead of from a dense inverse: the cost of a second factorization, and no n^2 memory
template <int DC, int DP>
static void schur_marginals_sparse_factor_t(slampp_hip_solver &s, CSchurState &S, const double *A)
{
	double *p_S = S.d_in_buf.p(), *p_r = S.d_in_buf.p() + size_t(S.n_in_blocks) * DC * DC;
	// (the covariance gathers read W of every observation and C^-1 of every landmark)
	schur_fill_t<DC, DP>(s, S, A, S.d_m_zero.p(), p_S, true, true, "marginals_assemble", []() {});
	if(s.p_allreduce)
		schur_sum_over_ranks_t<DC, DP>(s, S, p_S, true, true);
	s.Phase_Begin("marginals_factor");
	S.p_inner->p_flag_shared = s.d_flag.p();
	S.p_inner->b_leaf_linv_wanted = true; // (the inverse subset multiplies by inv(L_jj) of every column)
	S.p_inner->Enqueue_Sparse(p_S, p_r, true, true); // numeric factorization only
	S.p_inner->Ensure_Leaf_Inverses();
	s.Phase_End();
}

// the dense reduced system of the covariances assembled into d_m_S, factored, and inverted into d_m_Z.  Landmark shards: S is
// summed over the ranks as a whole buffer (the padding diagonal comes back as the number of ranks, which its decoupled
// rows do not mind)
template <int DC, int DP>
static void schur_marginals_dense_inverse_t(slampp_hip_solver &s, CSchurState &S, const double *A)
{
	hipStream_t st = s.stream;
	const int ld = S.Npad, n = S.N;
	if(!S.d_m_S.p()) {
		S.d_m_S.Alloc(size_t(ld) * ld);
		S.d_m_Z.Alloc(size_t(ld) * ld);
		S.d_m_invdiag.Alloc(size_t(ld / dense_NB) * dense_NB * dense_NB);
		const size_t n_zero = size_t(n) + size_t(S.np) * DP; // a whole right-hand side of zeros
		S.d_m_zero.Alloc(n_zero);
		SLAMPP_HIP_CHECK(hipMemsetAsync(S.d_m_zero.p(), 0, n_zero * sizeof(double), st));
	}
	double *p_S = S.d_m_S.p();
	schur_fill_t<DC, DP>(s, S, A, S.d_m_zero.p(), p_S, false, true, "marginals_assemble", []() {});
	if(s.p_allreduce)
		schur_sum_over_ranks_t<DC, DP>(s, S, p_S, false, false);
	s.Phase_Begin("marginals_factor");
	dense_cholesky(p_S, ld, n, S.d_m_invdiag.p(), s.d_flag.p(), st);
	s.Phase_End();
	s.Phase_Begin("marginals_inverse");
	dense_inverse_from_factor(p_S, ld, S.d_m_invdiag.p(), S.d_m_Z.p(), st);
	s.Phase_End();
}

// ---- what the other Schur units need from this one's kernels (schur_state.h), and the entry points ----

void schur_marginals_sparse_factor(slampp_hip_solver &s, CSchurState &S, const double *A)
{
	schur_dispatch(S.DC, S.DP, [&](auto dc, auto dp) { schur_marginals_sparse_factor_t<dc(), dp()>(s, S, A); });
}

void schur_marginals_dense_inverse(slampp_hip_solver &s, CSchurState &S, const double *A)
{
	schur_dispatch(S.DC, S.DP, [&](auto dc, auto dp) { schur_marginals_dense_inverse_t<dc(), dp()>(s, S, A); });
}

void schur_reduced_rhs_launch(CSchurState &S, const double *rhs, double *p_S, double *p_r, hipStream_t stream)
{
	schur_dispatch(S.DC, S.DP, [&](auto dc, auto dp) {
		hipLaunchKernelGGL((schur_rhs_kernel<dc(), dp()>), dim3(unsigned(S.nc)), dim3(64), 0, stream,
			S.d_cam_ptr.p(), S.d_cam_obs.p(), S.d_obs_pt.p(), S.N, S.d_W.p(), rhs, p_S, S.Npad, p_r);
	});
}

// the reference's Solve_PosDef_Blocky_MarginalPoses (LinearSolver_Schur.h:1956-2143): the landmarks' block of the
// system alone, dl = C^-1 eta_l, the pose part of the solution zeroed
void schur_enqueue_marginal_poses(slampp_hip_solver &s, const double *p_values_dev, double *p_rhs_dev)
{
	schur_invalidate_previous(s.p_schur);
	CSchurState &S = *s.p_schur;
	schur_dispatch(S.DC, S.DP, [&](auto dc, auto dp) { schur_enqueue_marginal_t<dc(), dp()>(s, S, p_values_dev, p_rhs_dev); });
}

void schur_enqueue(slampp_hip_solver &s, const double *p_values_dev, double *p_rhs_dev)
{
	CSchurState &S = *s.p_schur;
	schur_dispatch(S.DC, S.DP, [&](auto dc, auto dp) { schur_enqueue_t<dc(), dp()>(s, S, p_values_dev, p_rhs_dev); });
}

// a solve of this handle stores W and leaves the reduced system's factor for slampp_hip_solve_again (options "schur_keep",
// "schur_incremental"; never with landmark shards: the factor is of the summed system, W and C^-1 of this rank's landmarks)
bool schur_keeps_for_resolve(const slampp_hip_solver &s)
{
	return (s.n_schur_keep != 0 || s.n_schur_incremental != 0) && !s.p_allreduce && s.b_shard_primary;
}

} // namespace slampp

#include "preload.h"
SLAMPP_PRELOAD_UNIT(schur) // (the handle's bring-up thread loads this unit's code object: capi.hip)
