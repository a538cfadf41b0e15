// schur_tiles.hip -- landmark-major assembly of the reduced camera system S = A - U C^-1 U^T, r = x - U C^-1 l
// (steps 4-9 of CLinearSolver_Schur::Solve_PosDef_Blocky, /root/reference/include/slam/LinearSolver_Schur.h:1730-1830:
// InverseOf_BlockDiag, the two MultiplyToWith_FBS products, AddTo_FBS, PreMultiply_Add).
//
// The contribution lists of schur.hip read 288 bytes per (landmark, camera pair): a landmark seen by k cameras is read
// k (k + 1) / 2 times -- 1.44 GB at C4 for 0.58 GB of blocks, and the list kernel ran at the HBM traffic those re-reads
// generate.  Here every landmark is read once, by one of two kernels the host analysis (schur_tile_tables.cpp) picks:
//   runs   landmarks seen by exactly the same cameras (at least four of them): their products all land in the same blocks
//          of S, so a wave keeps the sums in matrix-core accumulators for a whole piece of the run (schur_run_kernel);
//   tiles  the other landmarks, sorted by their first two cameras and cut where they touch more than SCHUR_TILE_SLOTS
//          distinct blocks of S: a wave keeps a tile's blocks (and the right-hand sides of its cameras) in LDS and adds
//          every landmark's k (k + 1) / 2 products U_b W_a^T into them, one lane per (camera pair, row) (schur_tile_kernel).
// Either way the landmark's record [U_1 .. U_k | C | l] is loaded, C inverted, W = U C^-1 formed on the fly; the sums go
// to a partial array, and a last kernel adds up the partial blocks of every block of S in list order: no atomics on
// memory, the sum order is fixed by the analysis (bit-reproducible, like the lists).
// Landmarks with more cameras than a tile has room for that are in no run, and tiles whose landmarks share too little
// (fewer than three contributions per block: random visibility), stay with the contribution lists.
// SLAMPP_HIP_DEV_TILE_POINTS / SLAMPP_HIP_DEV_RUN_PIECE (environment, with SLAMPP_HIP_DEV=1: plan.h) are development knobs for the landmarks per tile / per run piece.
#include "schur_tiles.h"
#include "schur_state.h"

#include <algorithm>
#include <cstring>

namespace slampp {

#include "schur_device.inl"

__device__ __forceinline__ int64_t readlane64(int64_t v, int n_lane)
{
	return (int64_t(__builtin_amdgcn_readlane(int(v >> 32), n_lane)) << 32) | uint32_t(__builtin_amdgcn_readlane(int(v), n_lane));
}

__device__ __forceinline__ double readlane_f64(double v, int n_lane)
{
	return __longlong_as_double(readlane64(__double_as_longlong(v), n_lane));
}

__device__ __forceinline__ void wave_lds_fence()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int DC, int DP, int CAP, int NL>
__global__ void __launch_bounds__(64)
schur_tile_kernel(const int32_t *__restrict__ tile_ptr, const int32_t *__restrict__ tile_lm,
	const int64_t *__restrict__ tile_slot_ptr, const int64_t *__restrict__ pair_ptr, const uint8_t *__restrict__ lm_slot,
	const int64_t *__restrict__ ptr, int64_t nc, int64_t ubase, const double *__restrict__ A, const double *__restrict__ eta,
	int n, double *Cinv, double *W, int b_store, double *P, double *R, int *p_flag, int n_max_slots)
{
	enum { BLK = DC * DP, BB = DC * DC, MAXK = tile_max_k(CAP), GROUP = 4,
		GCAP = (MAXK * BLK > 320)? (MAXK * BLK + 63) / 64 * 64 : 320 };
	// LDS sized by the launch for the largest tile (a tile of ten blocks needs 3 kB, one of 64 blocks 21 kB: the waves a
	// CU holds hide the latency of the landmark loads)
	extern __shared__ __attribute__((aligned(16))) double s_dyn[];
	double *s_u = s_dyn, *s_w = s_u + GCAP;
	double *s_acc = s_w + GCAP, *s_r = s_acc + n_max_slots * BB;
	uint8_t *s_slot = (uint8_t*)(s_r + n_max_slots * DC), *s_tri = s_slot + 64;
	const int lane = threadIdx.x;
	const int64_t tile = blockIdx.x;
	const int lm0 = tile_ptr[tile], lm1 = tile_ptr[tile + 1];
	const int64_t slot0 = tile_slot_ptr[tile];
	const int n_slots = int(tile_slot_ptr[tile + 1] - slot0);
	for(int e = lane; e < n_slots * BB; e += 64)
		s_acc[e] = 0;
	for(int e = lane; e < n_slots * DC; e += 64)
		s_r[e] = 0;
	{
		// pair j = b (b + 1) / 2 + a of a landmark's cameras a <= b
		int b = 0;
		while((b + 1) * (b + 2) / 2 <= lane)
			++ b;
		s_tri[lane] = uint8_t((lane - b * (b + 1) / 2) | (b << 4));
	}
	const int64_t ptr_nc = ptr[nc];
	bool b_bad = false;
	for(int base = lm0; base < lm1; base += 64) {
		const int n_chunk = min(64, lm1 - base);
		// lane L prepares landmark base + L: where its record sits, C^-1, l
		int my_k = 0;
		int64_t my_rec = 0, my_pp = 0, my_o0 = 0;
		double ci[DP * DP], l[DP];
		#pragma unroll
		for(int i = 0; i < DP * DP; ++ i)
			ci[i] = 0;
		#pragma unroll
		for(int i = 0; i < DP; ++ i)
			l[i] = 0;
		if(lane < n_chunk) {
			const int64_t pt = tile_lm[base + lane];
			const int64_t k0 = ptr[nc + pt], k1 = ptr[nc + pt + 1];
			my_k = int(k1 - k0 - 1);
			my_o0 = k0 - ptr_nc - pt;
			my_rec = ubase + my_o0 * BLK + pt * (DP * DP);
			my_pp = pair_ptr[pt];
			double c[DP * DP];
			const double *C = A + my_rec + int64_t(my_k) * BLK;
			#pragma unroll
			for(int i = 0; i < DP * DP; ++ i)
				c[i] = C[i];
			if(!spd_inverse<DP>(c, ci))
				b_bad = true;
			#pragma unroll
			for(int i = 0; i < DP; ++ i)
				l[i] = eta[n + pt * DP + i];
			if(b_store) {
				#pragma unroll
				for(int i = 0; i < DP * DP; ++ i)
					Cinv[pt * (DP * DP) + i] = ci[i];
			}
		}
		// Landmarks are taken GROUP at a time: all their blocks are requested together, and the next group's while this
		// one is multiplied (a landmark's products take a fraction of a memory latency and a CU holds ten of these waves:
		// with one landmark in flight per wave the kernel ran at 1.5 TB/s).  The requests are straight-line code -- every
		// lane of every slot loads, lanes and slots with nothing to fetch re-read the group's first address -- because the
		// compiler puts a full s_waitcnt in front of a load it finds behind a branch.
		double v[GROUP][NL];
		uint8_t n_my_slot;
		int n_group, n_next = 0; // landmarks of the group in flight; first landmark after it
		auto Request = [&](int n_first) {
			const int i0 = min(n_first, n_chunk - 1);
			const int64_t rec0 = readlane64(my_rec, i0);
			int n_doubles = 0, n_group_pairs = 0;
			n_group = 0;
			#pragma unroll
			for(int g = 0; g < GROUP; ++ g) {
				const int ig = min(n_first + g, n_chunk - 1);
				const int k = __builtin_amdgcn_readlane(my_k, ig);
				const int64_t rec = readlane64(my_rec, ig);
				const bool b_in = n_group == g && n_first + g < n_chunk &&
					(g == 0 || (n_doubles + k * BLK <= GCAP && n_group_pairs + k * (k + 1) / 2 <= 64));
				#pragma unroll
				for(int m = 0; m < NL; ++ m)
					v[g][m] = A[(b_in && lane + 64 * m < k * BLK)? rec + lane + 64 * m : rec0];
				n_doubles += b_in? k * BLK : 0;
				n_group_pairs += b_in? k * (k + 1) / 2 : 0;
				n_group += b_in;
			}
			// the slots of consecutive landmarks of a tile are consecutive
			n_my_slot = lm_slot[readlane64(my_pp, i0) + ((lane < n_group_pairs)? lane : 0)];
			n_next = n_first + n_group;
		};
		Request(0);
		for(int i = 0; i < n_chunk;) {
			const int n_cur_group = n_group;
			{
				int n_off = 0, n_slot_num = 0;
				#pragma unroll
				for(int g = 0; g < GROUP; ++ g) {
					const int k = (g < n_cur_group)? __builtin_amdgcn_readlane(my_k, min(i + g, n_chunk - 1)) : 0;
					#pragma unroll
					for(int m = 0; m < NL; ++ m) {
						if(lane + 64 * m < k * BLK)
							s_u[n_off + lane + 64 * m] = v[g][m];
					}
					n_off += k * BLK;
					n_slot_num += k * (k + 1) / 2;
				}
				if(lane < n_slot_num)
					s_slot[lane] = n_my_slot;
			}
			wave_lds_fence();
			Request(n_next); // (past the chunk's end: an empty group, its loads re-read one address)
			int n_off = 0, n_pair_off = 0;
			for(int g = 0; g < n_cur_group; ++ g) {
				const int k = __builtin_amdgcn_readlane(my_k, i + g);
				const int n_pairs = k * (k + 1) / 2;
				const double *s_ug = s_u + n_off;
				double *s_wg = s_w + n_off;
				const uint8_t *s_slotg = s_slot + n_pair_off;
				double c_i[DP * DP], l_i[DP];
				#pragma unroll
				for(int t = 0; t < DP * DP; ++ t)
					c_i[t] = readlane_f64(ci[t], i + g);
				#pragma unroll
				for(int t = 0; t < DP; ++ t)
					l_i[t] = readlane_f64(l[t], i + g);
				const int64_t o0 = readlane64(my_o0, i + g);
				// W_o = U_o C^-1 and the right-hand side's share W_o l: one lane per (observation, row) -- ten observations of a
				// seven-dimensional camera are 70 rows: a second round (until round 4 the rows past 64 were left out: a wrong S
				// for Sim(3) landmarks seen by exactly ten cameras that went through a tile)
				for(int n_row0 = 0; n_row0 < k * DC; n_row0 += 64) {
					const int n_row = n_row0 + lane;
					if(n_row >= k * DC)
						continue;
					const int o = n_row / DC, r = n_row - o * DC;
					double u[DP], rv = 0;
					#pragma unroll
					for(int t = 0; t < DP; ++ t)
						u[t] = s_ug[o * BLK + r + t * DC];
					#pragma unroll
					for(int q = 0; q < DP; ++ q) {
						double w = 0;
						#pragma unroll
						for(int t = 0; t < DP; ++ t)
							w += u[t] * c_i[t + q * DP];
						s_wg[o * BLK + r + q * DC] = w;
						if(W)
							W[(o0 + o) * BLK + r + q * DC] = w;
						rv += w * l_i[q];
					}
					const int n_slot = s_slotg[o * (o + 3) / 2]; // pair (o, o)
					atomicAdd(&s_r[n_slot * DC + r], rv); // (cameras are distinct inside a landmark: no two lanes meet)
				}
				wave_lds_fence();
				// the products U_b W_a^T: one lane per (pair, row of the block)
				for(int n_first = 0; n_first < n_pairs * DC; n_first += 64) {
					const int n_task = n_first + lane;
					if(n_task < n_pairs * DC) {
						const int j = n_task / DC, r = n_task - j * DC;
						const int n_tri = s_tri[j], a = n_tri & 15, b = n_tri >> 4;
						double u[DP];
						#pragma unroll
						for(int t = 0; t < DP; ++ t)
							u[t] = s_ug[b * BLK + r + t * DC];
						double *p_acc = &s_acc[int(s_slotg[j]) * BB + r];
						const double *p_w = &s_wg[a * BLK];
						#pragma unroll
						for(int q = 0; q < DC; ++ q) {
							double f = 0;
							#pragma unroll
							for(int t = 0; t < DP; ++ t)
								f += u[t] * p_w[q + t * DC];
							atomicAdd(p_acc + q * DC, f);
						}
					}
				}
				n_off += k * BLK;
				n_pair_off += n_pairs;
			}
			wave_lds_fence(); // the next group overwrites the operands
			i += n_cur_group;
		}
	}
	if(b_bad)
		atomicOr(p_flag, 1);
	for(int e = lane; e < n_slots * BB; e += 64)
		P[slot0 * BB + e] = s_acc[e];
	for(int e = lane; e < n_slots * DC; e += 64)
		R[slot0 * DC + e] = s_r[e];
}

// ---- runs: landmarks seen by exactly the same cameras ----
// A run's products all land in the same k (k + 1) / 2 blocks of S, so they never leave the registers: for every landmark
// the wave multiplies [U_1; ..; U_k] (6k x 3) by [W_1; ..; W_k]^T on the matrix cores (v_mfma_f64_16x16x4, one landmark =
// one K step, the fourth k idle; the tiles above the diagonal are skipped) and only the sums over the run's landmarks
// are written, as partial blocks.  Observations are handled OB = 64 / DC at a time: a job is (piece of a run of at most
// 64 landmarks, block of OB row observations, block of OB column observations); up to OB cameras that is one job per
// piece, a landmark seen by 30 cameras takes six.  The right-hand side's share U C^-1 l is one FMA per landmark and
// row tile on the vector unit, reduced over the three k lanes at the end (diagonal jobs).
// The blocks of GROUP landmarks are fetched with coalesced loads, the next group's while this one is multiplied,
// and go through LDS into the fragment layout (lane = (row or column, k)).  Loading the fragments straight from memory
// -- eight 8-byte gathers per landmark over its 576-byte record -- cost 176 L1 accesses per landmark and ran at
// 216 us for C4; coalesced it is ten.
// b_quad (round 5): FOUR landmarks per matrix-core step instead of one.  The K dimension of v_mfma_f64_16x16x4 held the
// three coordinates of ONE landmark (and an idle fourth slot): per landmark the wave read C^-1, formed W's column and issued
// a full set of tiles, 131 vector instructions beside 10 matrix ones.  With K = four landmarks -- lane (m16, kk) works on
// landmark kk of a quad, and the three coordinates are three rounds of tiles, S += sum_j U(:, j) W(:, j)^T -- no slot is idle
// (9 matrix instructions per tile set and quad instead of 12), the lanes of different kk no longer read the same U values
// four times, and C^-1, C^-1 l and the masks are fetched once per quad and lane.
template <int DC, int DP, int NT, bool b_diag, bool b_prefix, bool b_quad = false> // b_prefix: some landmarks of the job end before the run's list does
__global__ void __launch_bounds__(64)
schur_run_kernel(const TRunJob *__restrict__ jobs, const int32_t *__restrict__ run_lm, const int64_t *__restrict__ run_rec,
	const int32_t *__restrict__ run_k, int64_t ubase, const double *__restrict__ A, const double *__restrict__ eta, int n, double *Cinv, double *W, int b_store,
	double *P, double *R, int *p_flag)
{
	enum { BLK = DC * DP, BB = DC * DC, OB = 64 / DC, OBT = (NT * 16 / DC < OB)? NT * 16 / DC : OB, // observations per block here
		SEG = OBT * BLK, NLD = (SEG + 63) / 64,
		GROUP = (NT <= 2)? 8 : (b_diag? 4 : 2) }; // (off-diagonal jobs of three or four tiles a side keep 16 accumulator tiles: with four landmarks in
	// flight the requested values were parked in accumulator registers one by one, a wait behind every load -- round 4)
	typedef double v4f64 __attribute__((ext_vector_type(4)));
	__shared__ double s_ci[64 * DP * DP];
	__shared__ double s_z[64 * DP];
	__shared__ double s_u[GROUP][b_diag? SEG : 2 * SEG]; // [blocks of the row observations | of the column observations, if they are others]
	__shared__ int s_kown[b_quad? 64 : 1];       // b_quad: every landmark's own number of observations (0 past the piece's end) ...
	__shared__ int64_t s_o0[b_quad? 64 : 1];     // ... and its first observation (where its W goes)
	static_assert(!b_quad || GROUP % 4 == 0, "quads of landmarks");
	const int lane = threadIdx.x, kk = lane >> 4, m16 = lane & 15;
	const TRunJob job = jobs[blockIdx.x];
	const int k = job.n_k, n_rb = job.n_rb, n_cb = job.n_cb, n_points_all = job.n_points;
	int n_points = min(n_points_all, 64), n_sub_first = job.n_first; // (round 5) a job takes its landmarks 64 at a time -- lane L prepares landmark L of a sub-piece -- and keeps its sums across sub-pieces: longer pieces, fewer partial blocks
	const int n_len_a = min(OB, k - n_rb * OB) * BLK, n_len_b = min(OB, k - n_cb * OB) * BLK; // doubles of the two segments
	// what this lane feeds the matrix cores: element (row, kk) of the U rows, element (kk, column) of the W columns
	int n_off_a[NT], n_off_b[NT], n_obs_a[NT], n_obs_b[NT];
	bool b_a[NT], b_b[NT];
	#pragma unroll
	for(int t = 0; t < NT; ++ t) {
		const int n_line = t * 16 + m16, o = n_line / DC, e = n_line - o * DC;
		b_a[t] = o < OB && n_rb * OB + o < k && (b_quad || kk < DP);
		n_off_a[t] = b_a[t]? o * BLK + (b_quad? 0 : kk * DC) + e : 0; // (b_quad: element (row, 0); the lane reads all three columns)
		b_b[t] = o < OB && n_cb * OB + o < k && (b_quad || kk < DP);
		n_off_b[t] = (b_b[t]? o * BLK + e : 0) + (b_diag? 0 : SEG);
		n_obs_a[t] = n_rb * OB + o;
		n_obs_b[t] = n_cb * OB + o;
	}
	const int kc = (kk < DP)? kk : 0;
	// lane L prepares landmark L of the piece: where its blocks are (the host wrote that down), C^-1 and C^-1 l
	// (round 4: a run may also hold landmarks whose camera list is a PREFIX of the run's -- tracks born at the same camera and
	// lost at different ones --: my_k is the landmark's own number of observations, what lies beyond it reads as zero)
	int64_t my_rec = 0, my_pt = 0;
	int my_k = k;
	v4f64 acc[NT][NT];
	double racc[NT];
	#pragma unroll
	for(int rt = 0; rt < NT; ++ rt) {
		racc[rt] = 0;
		#pragma unroll
		for(int ct = 0; ct < NT; ++ ct)
			acc[rt][ct] = v4f64{0, 0, 0, 0};
	}
	const bool b_store_w = W != 0 && b_diag;
	// requests of a group: straight-line code (lanes past a segment's end and slots past the piece's end re-read a valid
	// address), so that all of them are in flight together
	double va[GROUP][NLD], vb[b_diag? 1 : GROUP][NLD];
	const int64_t n_seg_a = int64_t(n_rb) * OB * BLK, n_seg_b = int64_t(n_cb) * OB * BLK;
	auto Request = [&](int n_first) {
		#pragma unroll
		for(int g = 0; g < GROUP; ++ g) {
			// (b_prefix: a landmark may end before the run's list does.  Its loads stay inside its own record -- U blocks and the C
			// block behind them -- and what they bring from beyond its last observation is never multiplied: the operands are
			// masked where they are read out of LDS.  A select on a value just requested, tried first, made the compiler wait
			// for every load in turn: 24 round trips per group instead of one.)
			const int n_lm = min(n_first + g, n_points - 1);
			const double *p_rec = A + readlane64(my_rec, n_lm);
			const int n_last = b_prefix? __builtin_amdgcn_readlane(my_k, n_lm) * BLK + DP * DP - 1 : 0x7fffffff;
			#pragma unroll
			for(int m = 0; m < NLD; ++ m) {
				va[g][m] = p_rec[min(int(n_seg_a) + ((lane + 64 * m < n_len_a)? lane + 64 * m : 0), n_last)];
				if(!b_diag)
					vb[g][m] = p_rec[min(int(n_seg_b) + ((lane + 64 * m < n_len_b)? lane + 64 * m : 0), n_last)];
			}
		}
	};
	bool b_bad = false;
	for(int n_sub = 0; n_sub < n_points_all; n_sub += 64) {
	n_points = min(n_points_all - n_sub, 64);
	n_sub_first = job.n_first + n_sub;
	my_rec = 0; my_pt = 0; my_k = k;
	if(lane < n_points) {
		my_pt = run_lm[n_sub_first + lane];
		my_rec = run_rec[n_sub_first + lane];
		my_k = run_k[n_sub_first + lane];
	}
	if(n_sub)
		wave_lds_fence(); // the last group of the sub-piece before has been read: s_ci, s_z (and the quads' tables) can go
	Request(0); // (flies while the landmark blocks are inverted)
	if(lane < n_points) {
		const int64_t pt = my_pt;
		double c[DP * DP], ci[DP * DP];
		const double *C = A + my_rec + int64_t(my_k) * BLK;
		#pragma unroll
		for(int i = 0; i < DP * DP; ++ i)
			c[i] = C[i];
		if(!spd_inverse<DP>(c, ci))
			b_bad = true;
		#pragma unroll
		for(int i = 0; i < DP * DP; ++ i)
			s_ci[lane * (DP * DP) + i] = ci[i];
		#pragma unroll
		for(int t = 0; t < DP; ++ t) {
			double z = 0;
			#pragma unroll
			for(int i = 0; i < DP; ++ i)
				z += ci[t + i * DP] * eta[n + pt * DP + i];
			s_z[lane * DP + t] = z; // C^-1 l
		}
		if(b_store && n_rb == 0 && n_cb == 0) {
			#pragma unroll
			for(int i = 0; i < DP * DP; ++ i)
				Cinv[pt * (DP * DP) + i] = ci[i];
		}
	}
	if constexpr(b_quad) {
		s_kown[lane] = (lane < n_points)? my_k : 0;
		s_o0[lane] = (lane < n_points)? (my_rec - ubase - my_pt * (DP * DP)) / BLK : 0;
	}
	for(int p0 = 0; p0 < n_points; p0 += GROUP) {
		wave_lds_fence(); // the previous group's fragments have been read (and, the first time, s_ci / s_z written)
		#pragma unroll
		for(int g = 0; g < GROUP; ++ g) {
			#pragma unroll
			for(int m = 0; m < NLD; ++ m) {
				if(lane + 64 * m < n_len_a)
					s_u[g][lane + 64 * m] = va[g][m];
				if(!b_diag && lane + 64 * m < n_len_b)
					s_u[g][(b_diag? 0 : SEG) + lane + 64 * m] = vb[b_diag? 0 : g][m];
			}
		}
		wave_lds_fence();
		Request(p0 + GROUP); // (past the end: re-reads the last landmark)
		if constexpr(b_quad) {
			#pragma unroll
			for(int q0 = 0; q0 < GROUP; q0 += 4) {
				if(p0 + q0 >= n_points) // (wave-uniform: the whole quad lies past the piece's end)
					break;
				const int g = q0 + kk;                        // this lane's landmark of the quad
				const int p = min(p0 + g, n_points - 1);
				const int n_k_lane = (p0 + g < n_points)? (b_prefix? s_kown[p] : k) : 0; // observations of this lane's landmark (0: no landmark)
				double ci[DP * DP], z[DP];
				#pragma unroll
				for(int i = 0; i < DP * DP; ++ i)
					ci[i] = s_ci[p * (DP * DP) + i];
				#pragma unroll
				for(int j = 0; j < DP; ++ j)
					z[j] = s_z[p * DP + j];
				const double *su = &s_u[0][0] + g * (b_diag? SEG : 2 * SEG);
				double ua[NT][DP], wb[NT][DP];
				bool b_wb[NT];
				#pragma unroll
				for(int t = 0; t < NT; ++ t) {
					const bool b_row = b_a[t] && n_obs_a[t] < n_k_lane;
					double u[DP], v[DP];
					#pragma unroll
					for(int j = 0; j < DP; ++ j) {
						u[j] = su[n_off_a[t] + j * DC];
						ua[t][j] = b_row? u[j] : 0.0;
						racc[t] += ua[t][j] * z[j];
					}
					#pragma unroll
					for(int j = 0; j < DP; ++ j)
						v[j] = b_diag? u[j] : su[n_off_b[t] + j * DC];
					b_wb[t] = b_b[t] && n_obs_b[t] < n_k_lane;
					#pragma unroll
					for(int jj = 0; jj < DP; ++ jj) {
						double w = 0;
						#pragma unroll
						for(int i = 0; i < DP; ++ i)
							w += v[i] * ci[i + jj * DP]; // W(q, jj) = sum_i U(q, i) C^-1(i, jj)
						wb[t][jj] = b_wb[t]? w : 0.0;
					}
				}
				// (b_prefix: the longest landmark of the quad says how many row tiles are not all zeros)
				int n_k_quad = k;
				if(b_prefix) {
					n_k_quad = 0;
					#pragma unroll
					for(int i = 0; i < 4; ++ i)
						n_k_quad = max(n_k_quad, (p0 + q0 + i < n_points)? __builtin_amdgcn_readlane(my_k, min(p0 + q0 + i, n_points - 1)) : 0);
				}
				const int n_rt_own = b_prefix? (min(n_k_quad - n_rb * OB, int(OB)) * DC + 15) / 16 : NT;
				#pragma unroll
				for(int j = 0; j < DP; ++ j) {
					#pragma unroll
					for(int rt = 0; rt < NT; ++ rt) {
						if(b_prefix && rt >= n_rt_own) // (wave-uniform)
							continue;
						#pragma unroll
						for(int ct = 0; ct < NT; ++ ct) {
							if(ct <= rt || !b_diag)
								acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(ua[rt][j], wb[ct][j], acc[rt][ct], 0, 0, 0);
						}
					}
				}
				if(b_store_w) {
					const int64_t o0 = s_o0[p];
					#pragma unroll
					for(int t = 0; t < NT; ++ t) {
						if(b_wb[t]) {
							const int n_line = t * 16 + m16, o = n_line / DC, q = n_line - o * DC;
							#pragma unroll
							for(int jj = 0; jj < DP; ++ jj)
								W[(o0 + n_obs_b[t]) * BLK + q + jj * DC] = wb[t][jj];
						}
					}
				}
			}
		} else {
			#pragma unroll
			for(int g = 0; g < GROUP; ++ g) {
				const int p = min(p0 + g, n_points - 1);
				const bool b_live = p0 + g < n_points;
				const int n_k_own = b_prefix? __builtin_amdgcn_readlane(my_k, p) : k; // observations of this landmark
				double cik[DP], wb[NT], ua[NT];
				#pragma unroll
				for(int j = 0; j < DP; ++ j)
					cik[j] = s_ci[p * (DP * DP) + j + kc * DP];
				const double z = s_z[p * DP + kc];
				#pragma unroll
				for(int t = 0; t < NT; ++ t) {
					const double u = s_u[g][n_off_a[t]];
					ua[t] = (b_a[t] && b_live && (!b_prefix || n_obs_a[t] < n_k_own))? u : 0.0;
					racc[t] += ua[t] * z;
					double w = 0;
					#pragma unroll
					for(int j = 0; j < DP; ++ j)
						w += s_u[g][n_off_b[t] + j * DC] * cik[j]; // W(q, kk) = sum_j U(q, j) C^-1(j, kk)
					wb[t] = (b_b[t] && (!b_prefix || n_obs_b[t] < n_k_own))? w : 0.0;
				}
				// (b_prefix: a landmark that ends inside the row block fills only the first tiles of rows -- and, on the diagonal, of
				// columns --: the others would multiply zeros, and these kernels spend 27 - 36 % of the fp64 matrix peak as it is)
				const int n_rt_own = b_prefix? (min(n_k_own - n_rb * OB, int(OB)) * DC + 15) / 16 : NT;
				#pragma unroll
				for(int rt = 0; rt < NT; ++ rt) {
					if(b_prefix && rt >= n_rt_own) // (wave-uniform)
						continue;
					#pragma unroll
					for(int ct = 0; ct < NT; ++ ct) {
						if(ct <= rt || !b_diag)
							acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(ua[rt], wb[ct], acc[rt][ct], 0, 0, 0);
					}
				}
				if(b_store_w && b_live) {
					const int64_t o0 = (readlane64(my_rec, p) - ubase - readlane64(my_pt, p) * (DP * DP)) / BLK; // first observation of the landmark
					#pragma unroll
					for(int t = 0; t < NT; ++ t) {
						if(b_b[t] && n_obs_b[t] < n_k_own) {
							const int n_line = t * 16 + m16, o = n_line / DC, q = n_line - o * DC;
							W[(o0 + n_obs_b[t]) * BLK + q + kk * DC] = wb[t];
						}
					}
				}
			}
		}
	}
	} // (sub-pieces)
	if(b_bad)
		atomicOr(p_flag, 1);
	// lane l holds the elements ((l >> 4) + 4 reg, l & 15) of every 16 x 16 tile
	const int n_kb_c = min(OB, k - n_cb * OB); // observations of the column block
	#pragma unroll
	for(int rt = 0; rt < NT; ++ rt) {
		#pragma unroll
		for(int reg = 0; reg < 4; ++ reg) {
			const int n_row = rt * 16 + 4 * reg + kk, ob = n_row / DC, r = n_row - ob * DC;
			if(ob >= OB || n_rb * OB + ob >= k)
				continue;
			#pragma unroll
			for(int ct = 0; ct < NT; ++ ct) {
				const int n_col = ct * 16 + m16, oa = n_col / DC, q = n_col - oa * DC;
				if(oa >= OB || n_cb * OB + oa >= k || (b_diag && oa > ob))
					continue;
				const int64_t n_slot = job.n_pbase + (b_diag? ob * (ob + 1) / 2 + oa : ob * n_kb_c + oa);
				P[n_slot * BB + r + q * DC] = acc[rt][ct][reg];
			}
		}
	}
	if(b_diag) { // the right-hand side's share of row (rt, m16): the sum over the k lanes
		#pragma unroll
		for(int rt = 0; rt < NT; ++ rt) {
			double f = racc[rt];
			f += __shfl_down(f, 32);
			f += __shfl_down(f, 16);
			const int n_row = rt * 16 + m16, ob = n_row / DC, r = n_row - ob * DC;
			if(kk == 0 && ob < OB && n_rb * OB + ob < k)
				R[(job.n_pbase + ob * (ob + 3) / 2) * DC + r] = f;
		}
	}
}

// one wave per block of S that has partial blocks: S -= their sum, in list order; the diagonal blocks also bring the
// partial right-hand sides of their camera (lanes DC^2 .. DC^2 + DC - 1)
template <int DC>
__global__ void __launch_bounds__(64)
schur_tile_reduce_kernel(const int64_t *__restrict__ rb_ptr, const int32_t *__restrict__ rb_part,
	const int32_t *__restrict__ rb_sb, const int32_t *__restrict__ sb_row, const int32_t *__restrict__ sb_col,
	const double *__restrict__ P, const double *__restrict__ R, double *S, int ld, const int64_t *__restrict__ p_dst, double *p_r)
{
	enum { BB = DC * DC };
	const int64_t i = blockIdx.x;
	const int lane = threadIdx.x;
	const int64_t sb = rb_sb[i];
	const int64_t n_row = sb_row[sb], n_col = sb_col[sb];
	if constexpr(DC == 6) {
		// (round 5) 16 bytes a lane: 18 lanes hold a partial block, so one request brings THREE of them (lanes 0 .. 53) and the three
		// partial right-hand sides of a diagonal block beside them (lanes 54 .. 62, 3 lanes each): a third of the requests of the
		// one-element-a-lane form below, and three times the bytes in flight.  Every lane group adds up every third partial block
		// of the list, in list order; the three sums meet at the end: still a fixed order.
		typedef double v2f64 __attribute__((ext_vector_type(2)));
		const bool b_blk = lane < 54, b_rhs_lane = lane >= 54 && lane < 63 && n_row == n_col;
		const int g = b_blk? lane / 18 : (lane - 54) / 3, q = b_blk? lane - 18 * g : (lane - 54) - 3 * g; // partial block of the request, pair of elements
		const double *p_src = b_blk? P + 2 * q : R + 2 * ((lane < 63)? q : 0);
		const int n_stride = b_blk? BB : DC;
		v2f64 f = {0, 0};
		for(int64_t e0 = rb_ptr[i], e1 = rb_ptr[i + 1]; e0 < e1; e0 += 64) {
			const int n_here = int(min(int64_t(64), e1 - e0));
			const int n_my = rb_part[e0 + min(lane, n_here - 1)];
			for(int j0 = 0; j0 < n_here; j0 += 24) {
				v2f64 v[8];
				#pragma unroll
				for(int u = 0; u < 8; ++ u) {
					const int j = j0 + 3 * u;
					const int i0 = __builtin_amdgcn_readlane(n_my, min(j, n_here - 1)), i1 = __builtin_amdgcn_readlane(n_my, min(j + 1, n_here - 1)),
						i2 = __builtin_amdgcn_readlane(n_my, min(j + 2, n_here - 1));
					const int n_idx = (g == 0)? i0 : (g == 1)? i1 : i2;
					v[u] = *reinterpret_cast<const v2f64*>(p_src + int64_t(n_idx) * n_stride);
				}
				#pragma unroll
				for(int u = 0; u < 8; ++ u) {
					if(j0 + 3 * u + g < n_here)
						f += v[u];
				}
			}
		}
		// lane q of the first group collects the other two (the right-hand side lanes likewise, three lanes apart)
		const int n_from1 = b_blk? lane + 18 : lane + 3, n_from2 = b_blk? lane + 36 : lane + 6;
		const double f1x = __shfl(f.x, n_from1 & 63), f1y = __shfl(f.y, n_from1 & 63), f2x = __shfl(f.x, n_from2 & 63), f2y = __shfl(f.y, n_from2 & 63);
		f.x = (f.x + f1x) + f2x;
		f.y = (f.y + f1y) + f2y;
		if(lane < 18) {
			#pragma unroll
			for(int h = 0; h < 2; ++ h) {
				const int n_el = 2 * lane + h, r = n_el % DC, qc = n_el / DC;
				const size_t idx = p_dst? size_t(p_dst[sb]) + qc + r * DC : size_t(n_row * DC + r) + size_t(n_col * DC + qc) * ld;
				S[idx] -= h? f.y : f.x;
			}
		} else if(b_rhs_lane && lane < 57) {
			#pragma unroll
			for(int h = 0; h < 2; ++ h) {
				const int64_t c = n_row * DC + 2 * (lane - 54) + h;
				if(p_r)
					p_r[c] -= h? f.y : f.x;
				else
					S[size_t(ld - 1) + size_t(c) * ld] -= h? f.y : f.x;
			}
		}
		return;
	}
	const bool b_block = lane < BB, b_rhs = lane >= BB && lane < BB + DC && n_row == n_col;
	// the list's indices 64 at a time with one coalesced load, then eight partial blocks in flight at once (one after
	// the other a block with 36 partials -- Venice-like visibility -- was 36 dependent round trips: 156 us for that kernel);
	// the sum is still taken in list order
	const int n_el = b_block? lane : (b_rhs? lane - BB : 0); // (the other lanes re-read a valid element)
	const double *p_src = b_block? P : R;
	const int n_stride = b_block? BB : DC;
	double f = 0;
	for(int64_t e0 = rb_ptr[i], e1 = rb_ptr[i + 1]; e0 < e1; e0 += 64) {
		const int n_here = int(min(int64_t(64), e1 - e0));
		const int n_my = rb_part[e0 + min(lane, n_here - 1)];
		for(int j0 = 0; j0 < n_here; j0 += 8) {
			double v[8];
			#pragma unroll
			for(int u = 0; u < 8; ++ u)
				v[u] = p_src[int64_t(__builtin_amdgcn_readlane(n_my, min(j0 + u, n_here - 1))) * n_stride + n_el];
			#pragma unroll
			for(int u = 0; u < 8; ++ u)
				f += (j0 + u < n_here)? v[u] : 0.0;
		}
	}
	if(b_block) {
		const int r = lane % DC, q = lane / DC;
		const size_t idx = p_dst? size_t(p_dst[sb]) + q + r * DC : size_t(n_row * DC + r) + size_t(n_col * DC + q) * ld;
		S[idx] -= f;
	} else if(b_rhs) {
		const int64_t c = n_row * DC + (lane - BB);
		if(p_r)
			p_r[c] -= f;
		else
			S[size_t(ld - 1) + size_t(c) * ld] -= f;
	}
}

template <int DC, int DP>
static void tiles_enqueue_t(const CSchurTiles &T, const int64_t *ptr, int64_t nc, int64_t ubase, const double *A, const double *eta,
	int n, double *Cinv, double *p_W, bool b_store, const int32_t *sb_row, const int32_t *sb_col, double *S, int ld,
	const int64_t *p_dst, double *p_r, int *p_flag, hipStream_t stream)
{
	{
		const TRunJob *p_jobs = T.d_run_jobs.p();
#define LAUNCH_RUNS_Q(NT, DIAG, PFX, QUAD) hipLaunchKernelGGL((schur_run_kernel<DC, DP, NT, DIAG != 0, PFX != 0, QUAD>), \
			dim3(unsigned(T.n_run_jobs[NT][DIAG][PFX])), dim3(64), 0, stream, p_jobs + T.n_run_job_first[NT][DIAG][PFX], T.d_run_lm.p(), \
			T.d_run_rec.p(), T.d_run_k.p(), ubase, A, eta, n, Cinv, p_W, int(b_store), T.d_P.p(), T.d_R.p(), p_flag)
		// (run_launch_quad says which jobs take quads of landmarks: never the off-diagonal jobs of three and four tiles a side,
		// whose quad form is not instantiated)
#define LAUNCH_RUNS(NT, DIAG, PFX) do { if(T.n_run_jobs[NT][DIAG][PFX]) { if(run_launch_quad(NT, DIAG != 0)) LAUNCH_RUNS_Q(NT, DIAG, PFX, (NT <= 2 || DIAG)); \
			else LAUNCH_RUNS_Q(NT, DIAG, PFX, false); } } while(0)
#define LAUNCH_RUNS_D(NT, DIAG) do { LAUNCH_RUNS(NT, DIAG, 0); LAUNCH_RUNS(NT, DIAG, 1); } while(0)
		LAUNCH_RUNS_D(1, 1);
		LAUNCH_RUNS_D(2, 1);
		LAUNCH_RUNS_D(3, 1);
		LAUNCH_RUNS_D(4, 1);
		LAUNCH_RUNS_D(1, 0);
		LAUNCH_RUNS_D(2, 0);
		LAUNCH_RUNS_D(3, 0);
		LAUNCH_RUNS_D(4, 0);
#undef LAUNCH_RUNS_D
#undef LAUNCH_RUNS
#undef LAUNCH_RUNS_Q
	}
	if(T.n_tiles) {
	enum { BLK = DC * DP, MAXK = tile_max_k(SCHUR_TILE_SLOTS), OPS = (MAXK * BLK > 320)? (MAXK * BLK + 63) / 64 * 64 : 320,
		NL_MAX = (MAXK * BLK + 63) / 64 };
	const size_t n_lds = (2 * OPS + size_t(T.n_max_slots) * (DC * DC + DC)) * sizeof(double) + 128;
	const int n_loads = tile_launch_loads(DC, DP, T.n_max_k); // 64-lane loads that fetch the blocks of the largest landmark
#define LAUNCH_TILES(NL) hipLaunchKernelGGL((schur_tile_kernel<DC, DP, SCHUR_TILE_SLOTS, (NL <= NL_MAX)? NL : NL_MAX>), \
		dim3(unsigned(T.n_tiles)), dim3(64), n_lds, stream, T.d_tile_ptr.p(), T.d_tile_lm.p(), T.d_tile_slot_ptr.p(), \
		T.d_pair_ptr.p(), T.d_lm_slot.p(), ptr, nc, ubase, A, eta, n, Cinv, p_W, int(b_store), T.d_P.p(), T.d_R.p(), p_flag, \
		int(T.n_max_slots))
	if(n_loads <= 1)
		LAUNCH_TILES(1);
	else if(n_loads == 2)
		LAUNCH_TILES(2);
	else if(n_loads == 3)
		LAUNCH_TILES(3);
	else
		LAUNCH_TILES(4);
#undef LAUNCH_TILES
	}
	if(T.n_rb) // (landmarks nobody observes have no blocks of S to reduce)
		hipLaunchKernelGGL((schur_tile_reduce_kernel<DC>), dim3(unsigned(T.n_rb)), dim3(64), 0, stream,
		T.d_rb_ptr.p(), T.d_rb_part.p(), T.d_rb_sb.p(), sb_row, sb_col, T.d_P.p(), T.d_R.p(), S, ld, p_dst, p_r);
}

void schur_tiles_join(CSchurTiles &T)
{
	if(!T.p_run_upload)
		return;
	std::shared_ptr<TRunUpload> p_up;
	p_up.swap(T.p_run_upload);
	if(p_up->t.joinable())
		p_up->t.join();
	if(p_up->p_error)
		std::rethrow_exception(p_up->p_error);
}

void schur_tiles_enqueue(const CSchurTiles &T, int DC, int DP, const int64_t *ptr, int64_t nc, int64_t ubase, const double *A,
	const double *eta, int n, double *Cinv, double *p_W, bool b_store, const int32_t *sb_row, const int32_t *sb_col,
	double *S, int ld, const int64_t *p_dst, double *p_r, int *p_flag, hipStream_t stream)
{
	schur_dispatch(DC, DP, [&](auto dc, auto dp) {
		tiles_enqueue_t<dc(), dp()>(T, ptr, nc, ubase, A, eta, n, Cinv, p_W, b_store, sb_row, sb_col, S, ld, p_dst, p_r, p_flag, stream);
	});
}

// ---------------------------------------------------------------------------------------------
// host analysis: the builders of schur_tile_tables.cpp, and what they made on its way to the device
// ---------------------------------------------------------------------------------------------

// the run tables go to the device beside the rest of this analysis and of the caller's (19 ms of C5's cold call -- 50 MB out
// of pageable vectors --; schur_tiles_join waits for them).  The thread owns what it reads.
static void start_run_upload(CSchurTiles &T, const SchurTileTables &r_tables, const SchurStructure &r_s, hipStream_t stream)
{
	int n_device = 0;
	SLAMPP_HIP_CHECK(hipGetDevice(&n_device));
	T.p_run_upload = std::make_shared<TRunUpload>();
	TRunUpload *p_up = T.p_run_upload.get();
	p_up->p_tables = r_tables.p_runs;
	CSchurTiles *p_tiles = &T;
	const SchurStructure s = r_s;
	auto Upload_Runs = [p_up, p_tiles, n_device, stream, s]() {
		try {
			SLAMPP_HIP_CHECK(hipSetDevice(n_device));
			const SchurRunTables &r_runs = *p_up->p_tables;
			p_tiles->d_run_jobs.Upload(r_runs.jobs, stream);
			p_tiles->d_run_lm.Upload(r_runs.run_lm, stream);
			p_tiles->d_run_k.Upload(r_runs.run_k, stream);
			raw_vector<int64_t> run_rec(r_runs.run_lm.size());
			schur_run_records(run_rec.data(), r_runs.run_lm.data(), int64_t(run_rec.size()), s); // (eight threads: the analysis waits for this thread at its end)
			p_tiles->d_run_rec.Upload(run_rec, stream);
			SLAMPP_HIP_CHECK(hipStreamSynchronize(stream)); // (run_rec lives in this scope)
		} catch(...) {
			p_up->p_error = std::current_exception();
		}
	};
	if(r_tables.p_runs->run_lm.size() >= (size_t(1) << 18))
		p_up->t = std::thread(Upload_Runs);
	else
		Upload_Runs(); // (a small system: a thread's start-up is what it would save)
}

void schur_tiles_build(CSchurTiles &T, int n_mode, int DC, int DP, int64_t nc, int64_t np, const int64_t *ptr, const int32_t *brow,
	const std::vector<int32_t> &sb_row, const std::vector<int32_t> &sb_col, int64_t n_ablocks, hipStream_t stream)
{
	const SchurStructure s = {DC, DP, nc, np, ptr, brow, n_ablocks};
	SchurTileTables tables;
	const bool b_in_use = schur_tile_routes(tables, n_mode, s);
	T.n_all_pairs = tables.n_all_pairs;
	T.n_prefix_points = tables.n_prefix_points;
	if(!b_in_use)
		return; // the lists keep everything
	start_run_upload(T, tables, s, stream); // (the routes are decided: the run tables leave beside the lists below)
	for(size_t i = 0; i < tables.trash.size(); ++ i)
		T.trash.emplace_back(std::move(tables.trash[i])); // (the caller frees them behind the analysis: schur_setup.hip)
	tables.trash.clear();
	memcpy(T.n_run_jobs, tables.n_run_jobs, sizeof(T.n_run_jobs));
	memcpy(T.n_run_job_first, tables.n_run_job_first, sizeof(T.n_run_job_first));
	T.n_tiles = tables.n_tiles;
	T.n_slots = tables.n_slots;
	T.n_run_points = tables.n_run_points;
	T.n_tile_points = tables.n_tile_points;
	T.n_list_points = tables.n_list_points;
	T.n_tile_pairs = tables.n_tile_pairs;

	schur_tile_reduce_lists(tables, s, sb_row, sb_col);
	T.n_max_slots = tables.n_max_slots;
	T.n_max_k = tables.n_max_k;
	T.n_rb = tables.n_rb;
	if(T.n_tiles) { // (the tile kernel's tables: 16 bytes per landmark that nobody reads where every landmark is in a run -- 32 MB of C5's cold call)
		T.d_tile_ptr.Upload(tables.tile_ptr, stream);
		T.d_tile_lm.Upload(tables.tile_lm, stream);
		T.d_tile_slot_ptr.Upload(tables.tile_slot_ptr, stream);
		T.d_pair_ptr.Upload(tables.pair_ptr, stream);
		T.d_lm_slot.Upload(tables.lm_slot, stream);
	}
	T.d_rb_ptr.Upload(tables.rb_ptr, stream);
	T.d_rb_part.Upload(tables.rb_part, stream);
	T.d_rb_sb.Upload(tables.rb_sb, stream);
	T.d_P.Alloc(size_t(T.n_slots) * DC * DC);
	T.d_R.Alloc(size_t(T.n_slots) * DC);
	tables.Phase("uploads (runs)");

	schur_tile_xlists(tables, s);
	if(T.n_list_points > 0) {
		T.b_hybrid = true;
		T.d_xpoints.Upload(tables.xpoints, stream);
		T.n_xobs = int64_t(tables.xcam_obs.size());
		T.n_xblocks = int64_t(tables.xsb_map.size());
		T.n_xentries = int64_t(tables.xent_a.size());
		T.d_xsb_ptr.Upload(tables.xsb_ptr, stream);
		T.d_xsb_map.Upload(tables.xsb_map, stream);
		T.d_xent_a.Upload(tables.xent_a, stream);
		T.d_xent_uoff.Upload(tables.xent_uoff, stream);
		T.d_xcam_ptr.Upload(tables.xcam_ptr, stream);
		T.d_xcam_obs.Upload(tables.xcam_obs, stream);
	}
	tables.Phase("lists of the rest");
	SLAMPP_HIP_CHECK(hipStreamSynchronize(stream)); // the host tables live on this stack frame
	tables.Phase("sync");
	T.b_enabled = true;
}

} // namespace slampp

#include "preload.h"
SLAMPP_PRELOAD_UNIT(schur_tiles) // (the handle's bring-up thread loads this unit's code object: capi.hip)
