// dense_tiles.hip -- tile-sparse, level-scheduled factorization of the dense top (see dense_chol.h), and the
// identity diagonal of its alignment gaps.  Kept in its own translation unit: the register allocation of the
// kernels in dense_chol.hip was seen to change (260 instead of 204 registers for the diagonal-tile kernel, one
// workgroup per CU instead of two) when these kernels were compiled next to them.
#include <hip/hip_runtime.h>
#include "dense_chol.h"
#include "plan.h"
#include "tile_schedule.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace slampp {

#include "dense_device.inl"

__global__ void dense_gap_kernel(double *M, int ld, const int32_t *__restrict__ p_positions, int n_positions)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if(i < n_positions)
		M[p_positions[i] + size_t(p_positions[i]) * ld] = 1.0;
}

void dense_prepare_gaps(double *M, int n_pad, const int32_t *p_positions_dev, int n_positions, hipStream_t stream)
{
	if(n_positions > 0)
		hipLaunchKernelGGL(dense_gap_kernel, dim3((n_positions + 63) / 64), dim3(64), 0, stream, M, n_pad, p_positions_dev, n_positions);
}

// ---- tile-sparse, level-scheduled variant (see dense_chol.h) ----
// target tile (ti, tj) -= sum over its source tile columns kt of L(ti, kt) L(tj, kt)^T
__device__ __forceinline__ void tile_update_body(double *M, int ld, const int4 t_tgt, const int *__restrict__ p_sources, double *Ps, double *Qs)
{
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int row0 = t_tgt.x * NB, colq = t_tgt.y * NB;
	const int lo = lane & 15, hi = lane >> 4;
	double cv[4][4];
	#pragma unroll
	for(int c = 0; c < 4; ++ c)
		#pragma unroll
		for(int reg = 0; reg < 4; ++ reg)
			cv[c][reg] = M[size_t(row0 + 16 * c + lo) + size_t(colq + 16 * wave + hi + 4 * reg) * ld];
	v4f64 acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
	TTileRegs t_p, t_q;
	int kt = p_sources[t_tgt.z];
	fetch_tile(t_p, M, ld, row0, kt * NB);
	fetch_tile(t_q, M, ld, colq, kt * NB);
	for(int e = t_tgt.z; e < t_tgt.w; ++ e) {
		if(e > t_tgt.z)
			__syncthreads(); // the previous source has been consumed
		stage_tile(Ps, t_p);
		stage_tile(Qs, t_q);
		__syncthreads();
		if(e + 1 < t_tgt.w) {
			kt = p_sources[e + 1];
			fetch_tile(t_p, M, ld, row0, kt * NB);
			fetch_tile(t_q, M, ld, colq, kt * NB);
		}
		tile_product(Ps, Qs, wave, lane, acc);
	}
	#pragma unroll
	for(int c = 0; c < 4; ++ c)
		#pragma unroll
		for(int reg = 0; reg < 4; ++ reg)
			M[size_t(row0 + 16 * c + lo) + size_t(colq + 16 * wave + hi + 4 * reg) * ld] = cv[c][reg] - acc[c][reg];
}

// the diagonal tiles of a level; behind them ride the updates of the level before that nothing in this level waits for
// (everything but the diagonal tiles of this level's columns): the launch every level has to wait for keeps one CU
// busy per tile, the riders give the rest of the chip its share of the level's work
__global__ void __launch_bounds__(256)
tile_potrf_kernel(double *M, int ld, int n, double *p_invdiag, int *p_flag, const int *__restrict__ p_tiles, int n_potrf,
	const int4 *__restrict__ p_riders, const int *__restrict__ p_sources)
{
	__shared__ double s_buf[(int(POTRF_LDS_DOUBLES) > 2 * NB * NB)? int(POTRF_LDS_DOUBLES) : 2 * NB * NB];
	if(int(blockIdx.x) >= n_potrf) {
		tile_update_body(M, ld, p_riders[int(blockIdx.x) - n_potrf], p_sources, s_buf, s_buf + NB * NB);
		return;
	}
	const int kb = p_tiles[blockIdx.x];
	potrf_diag_body<true, true>(M, ld, kb, n, p_invdiag + size_t(kb) * NB * NB, p_flag, s_buf);
}

// L(i,j) = A(i,j) inv(L_jj)^T; with t_pair.z set the workgroup also applies its tile to the diagonal tile of its row,
// A(i,i) -= L(i,j) L(i,j)^T -- the one update the next level's diagonal tile is waiting for, where this tile is its
// only source in this level (a chain of tile columns: the top of every separator tree)
__global__ void __launch_bounds__(512)
tile_trsm_kernel(double *M, int ld, const double *p_invdiag, const int4 *__restrict__ p_pairs)
{
	__shared__ double s_buf[2 * NB * NB];
	const int4 t_pair = p_pairs[blockIdx.x];
	trsm_tile_body8(M, ld, t_pair.x * NB, t_pair.y * NB, p_invdiag + size_t(t_pair.y) * NB * NB, t_pair.z != 0, s_buf, s_buf + NB * NB);
}

__global__ void __launch_bounds__(256)
tile_update_kernel(double *M, int ld, const int4 *__restrict__ p_targets, const int *__restrict__ p_sources)
{
	__shared__ double Ps[NB * NB];
	__shared__ double Qs[NB * NB];
	tile_update_body(M, ld, p_targets[blockIdx.x], p_sources, Ps, Qs);
}

void CTileSchedule::Free()
{
	if(d_potrf) (void)hipFree(d_potrf);
	if(d_trsm) (void)hipFree(d_trsm);
	if(d_tgt) (void)hipFree(d_tgt);
	if(d_src) (void)hipFree(d_src);
	if(d_back_diag) (void)hipFree(d_back_diag);
	if(d_back_carry) (void)hipFree(d_back_carry);
	if(d_riders) (void)hipFree(d_riders);
	d_potrf = 0; d_trsm = 0; d_tgt = 0; d_src = 0; d_back_diag = 0; d_back_carry = 0; d_riders = 0;
	n_bytes = 0;
	n_levels = 0;
	n_tiles = 0;
}

bool CTileSchedule::Build(int n_tile_num, const std::vector<char> &r_nonzero, hipStream_t stream)
{
	Free();
	// the tables are host code of their own (tile_schedule.cpp): here they are only uploaded
	const int TILE_RIDER_CHUNK = dev_knob("SLAMPP_HIP_DEV_RIDER_CHUNK", 4), TILE_RIDER_BUDGET = dev_knob("SLAMPP_HIP_DEV_RIDER_BUDGET", 1024);
	TTileTables tables;
	const bool b_tables = tile_schedule_tables(n_tile_num, r_nonzero, TILE_RIDER_CHUNK, TILE_RIDER_BUDGET, tables);
	n_tiles = tables.n_tiles;
	n_levels = tables.n_levels;
	level_potrf_ptr = tables.level_potrf_ptr;
	level_trsm_ptr = tables.level_trsm_ptr;
	level_tgt_ptr = tables.level_tgt_ptr;
	level_urgent_end = tables.level_urgent_end;
	rider_ptr = tables.rider_ptr;
	back_diag_ptr = tables.back_diag_ptr;
	back_carry_ptr = tables.back_carry_ptr;
	if(!b_tables)
		return false;
	static_assert(sizeof(TTileRec4) == sizeof(int4), "the records are uploaded as they are");
	const std::vector<int> &potrf = tables.potrf, &src = tables.src;
	const std::vector<TTileRec4> &trsm = tables.trsm, &tgt = tables.tgt, &riders = tables.riders, &back_diag = tables.back_diag,
		&back_carry = tables.back_carry;
	const size_t n_b4 = back_diag.size() * sizeof(int4), n_b5 = (back_carry.size() + 1) * sizeof(int4), n_b6 = (riders.size() + 1) * sizeof(int4);
	const size_t n_b0 = potrf.size() * sizeof(int), n_b1 = (trsm.size() + 1) * sizeof(int4),
		n_b2 = (tgt.size() + 1) * sizeof(int4), n_b3 = (src.size() + 1) * sizeof(int);
	if(hipMalloc((void**)&d_potrf, n_b0) != hipSuccess || hipMalloc((void**)&d_trsm, n_b1) != hipSuccess ||
	   hipMalloc((void**)&d_tgt, n_b2) != hipSuccess || hipMalloc((void**)&d_src, n_b3) != hipSuccess ||
	   hipMalloc((void**)&d_back_diag, n_b4) != hipSuccess || hipMalloc((void**)&d_back_carry, n_b5) != hipSuccess ||
	   hipMalloc((void**)&d_riders, n_b6) != hipSuccess) {
		(void)hipGetLastError();
		Free();
		return false;
	}
	bool b_ok = hipMemcpyAsync(d_potrf, potrf.data(), n_b0, hipMemcpyHostToDevice, stream) == hipSuccess;
	if(!trsm.empty())
		b_ok = b_ok && hipMemcpyAsync(d_trsm, trsm.data(), trsm.size() * sizeof(int4), hipMemcpyHostToDevice, stream) == hipSuccess;
	if(!tgt.empty())
		b_ok = b_ok && hipMemcpyAsync(d_tgt, tgt.data(), tgt.size() * sizeof(int4), hipMemcpyHostToDevice, stream) == hipSuccess;
	if(!src.empty())
		b_ok = b_ok && hipMemcpyAsync(d_src, src.data(), src.size() * sizeof(int), hipMemcpyHostToDevice, stream) == hipSuccess;
	if(!riders.empty())
		b_ok = b_ok && hipMemcpyAsync(d_riders, riders.data(), riders.size() * sizeof(int4), hipMemcpyHostToDevice, stream) == hipSuccess;
	b_ok = b_ok && hipMemcpyAsync(d_back_diag, back_diag.data(), n_b4, hipMemcpyHostToDevice, stream) == hipSuccess;
	if(!back_carry.empty())
		b_ok = b_ok && hipMemcpyAsync(d_back_carry, back_carry.data(), back_carry.size() * sizeof(int4), hipMemcpyHostToDevice, stream) == hipSuccess;
	b_ok = b_ok && hipStreamSynchronize(stream) == hipSuccess; // the host vectors live on this stack frame
	if(!b_ok) {
		(void)hipGetLastError();
		Free();
		return false;
	}
	n_bytes = n_b0 + n_b1 + n_b2 + n_b3 + n_b4 + n_b5 + n_b6;
	return true;
}

// zeroes the tiles of the schedule (the diagonal ones whole): what a step's assembly adds into; the other tiles are
// never written by anything that works from the schedule, so once zero they stay zero
__global__ void __launch_bounds__(256)
tile_zero_kernel(double *M, int ld, const int *__restrict__ p_potrf, int n_potrf, const int4 *__restrict__ p_trsm,
	const uint8_t *__restrict__ p_unit)
{
	int ti, tj;
	if(int(blockIdx.x) < n_potrf)
		ti = tj = p_potrf[blockIdx.x];
	else {
		const int4 t = p_trsm[int(blockIdx.x) - n_potrf];
		ti = t.x;
		tj = t.y;
	}
	const int r = (threadIdx.x & 31) * 2, c0 = threadIdx.x >> 5;
	#pragma unroll
	for(int i = 0; i < NB / 8; ++ i) {
		const int c = c0 + 8 * i;
		v2f64 v = {0, 0};
		if(ti == tj && p_unit && (c >> 1) == (r >> 1) && p_unit[tj * NB + c]) { // the identity of padding and gaps (own launches once)
			if(c & 1)
				v.y = 1.0;
			else
				v.x = 1.0;
		}
		*reinterpret_cast<v2f64*>(M + size_t(ti * NB + r) + size_t(tj * NB + c) * ld) = v;
	}
}

void tile_zero(const CTileSchedule &r_s, double *M, int n_pad, hipStream_t stream, const uint8_t *p_unit)
{
	const int n_potrf = r_s.level_potrf_ptr.back(), n_trsm = r_s.level_trsm_ptr.back();
	hipLaunchKernelGGL(tile_zero_kernel, dim3(n_potrf + n_trsm), dim3(256), 0, stream, M, n_pad, r_s.d_potrf, n_potrf, r_s.d_trsm, p_unit);
}

void tile_cholesky(const CTileSchedule &r_s, double *M, int n_pad, int n, double *p_invdiag, int *p_flag, hipStream_t stream)
{
	for(int l = 0; l < r_s.n_levels; ++ l) {
		const int p0 = r_s.level_potrf_ptr[l], p1 = r_s.level_potrf_ptr[l + 1];
		const int t0 = r_s.level_trsm_ptr[l], t1 = r_s.level_trsm_ptr[l + 1];
		const int g0 = r_s.level_tgt_ptr[l], gu = r_s.level_urgent_end[l];
		const int r0 = r_s.rider_ptr[l], r1 = r_s.rider_ptr[l + 1]; // the updates that ride in this level's diagonal launch
		if(p1 > p0 || r1 > r0) {
			hipLaunchKernelGGL(tile_potrf_kernel, dim3((p1 - p0) + (r1 - r0)), dim3(256), 0, stream, M, n_pad, n, p_invdiag, p_flag,
				r_s.d_potrf + p0, p1 - p0, r_s.d_riders + r0, r_s.d_src);
		}
		if(t1 > t0)
			hipLaunchKernelGGL(tile_trsm_kernel, dim3(t1 - t0), dim3(512), 0, stream, M, n_pad, p_invdiag, r_s.d_trsm + t0);
		if(gu > g0)
			hipLaunchKernelGGL(tile_update_kernel, dim3(gu - g0), dim3(256), 0, stream, M, n_pad, r_s.d_tgt + g0, r_s.d_src);
	}
}

// One launch of the backward substitution by levels (tile_backsolve).  Thread (c, part) = (t / 8, t % 8) holds the eight
// entries 2 part + 16 i + {0, 1} of column c of a tile, fetched as four 16-byte pairs: the eight threads of a column read
// whole 128-byte lines.  Everything a workgroup needs is requested before the first dependent step.
__global__ void __launch_bounds__(512)
tile_backsolve_kernel(const double *M, int ld, int n, const double *p_invdiag, double *z, double *x,
	const int4 *__restrict__ p_diag, int n_diag, const int4 *__restrict__ p_carry,
	const longlong2 *__restrict__ p_dst, double *p_w, double *p_x_out)
{
	enum { PARTS = 8, PER = NB / PARTS };
	__shared__ double s_x[NB];
	__shared__ double s_z[NB];
	const int t = threadIdx.x, c = t / PARTS, part = t % PARTS;
	const bool b_diag = int(blockIdx.x) < n_diag;
	const int4 rec = b_diag? p_diag[blockIdx.x] : p_carry[int(blockIdx.x) - n_diag];
	const int j = b_diag? rec.y : rec.x, k = b_diag? rec.x : rec.y; // z_k -= L(j,k)^T x_j (j < 0: nothing to subtract)
	double vl[PER], vi[PER];
	if(j >= 0) {
		const double *col = M + size_t(j * NB + 2 * part) + size_t(k * NB + c) * ld;
		#pragma unroll
		for(int i = 0; i < PER; i += 2) {
			const v2f64 v = *reinterpret_cast<const v2f64*>(col + PARTS * i);
			vl[i] = v.x;
			vl[i + 1] = v.y;
		}
	}
	if(b_diag) {
		const double *invL = p_invdiag + size_t(k) * NB * NB + c * NB + 2 * part;
		#pragma unroll
		for(int i = 0; i < PER; i += 2) {
			const v2f64 v = *reinterpret_cast<const v2f64*>(invL + PARTS * i);
			vi[i] = v.x;
			vi[i + 1] = v.y;
		}
	}
	double z_in = 0;
	if(t < NB) {
		const int q = k * NB + t;
		z_in = rec.z? ((q < n)? M[size_t(ld - 1) + size_t(q) * ld] : 0.0) : z[q];
		s_x[t] = (j >= 0)? x[j * NB + t] : 0.0;
	}
	__syncthreads();
	double upd = 0;
	if(j >= 0) {
		#pragma unroll
		for(int i = 0; i < PER; ++ i)
			upd += vl[i] * s_x[2 * part + PARTS * (i & ~1) + (i & 1)];
		upd += __shfl_xor(upd, 1);
		upd += __shfl_xor(upd, 2);
		upd += __shfl_xor(upd, 4);
	}
	// (c, part = 0) holds the sum of column c; the thread that fetched z_in[c] is thread c: hand over through LDS
	if(part == 0)
		s_z[c] = upd;
	__syncthreads();
	if(!b_diag) {
		if(t < NB)
			z[k * NB + t] = z_in - s_z[t];
		return;
	}
	if(t < NB)
		s_x[t] = z_in - s_z[t]; // z_k, complete (s_x is free: every read of x_j is behind the barrier above)
	__syncthreads();
	double sum = 0; // x_k[c] = sum_r inv(L_kk)[r][c] z_k[r]
	#pragma unroll
	for(int i = 0; i < PER; ++ i)
		sum += vi[i] * s_x[2 * part + PARTS * (i & ~1) + (i & 1)];
	sum += __shfl_xor(sum, 1);
	sum += __shfl_xor(sum, 2);
	sum += __shfl_xor(sum, 4);
	if(part == 0) {
		const int q = k * NB + c;
		x[q] = sum;
		if(p_dst) {
			const longlong2 d = p_dst[q];
			if(d.x >= 0) {
				p_w[d.x] = sum;
				p_x_out[d.y] = sum;
			}
		}
	}
}

void tile_backsolve(const CTileSchedule &r_s, const double *M, int n_pad, int n, const double *p_invdiag, double *p_z,
	double *p_x, hipStream_t stream, const longlong2 *p_dst, double *p_w, double *p_x_out)
{
	for(int q = 0; q < r_s.n_levels; ++ q) {
		const int d0 = r_s.back_diag_ptr[q], d1 = r_s.back_diag_ptr[q + 1];
		const int c0 = r_s.back_carry_ptr[q], c1 = r_s.back_carry_ptr[q + 1];
		if(d1 - d0 + c1 - c0 > 0) {
			hipLaunchKernelGGL(tile_backsolve_kernel, dim3((d1 - d0) + (c1 - c0)), dim3(512), 0, stream, M, n_pad, n, p_invdiag,
				p_z, p_x, r_s.d_back_diag + d0, d1 - d0, r_s.d_back_carry + c0, p_dst, p_w, p_x_out);
		}
	}
}

} // namespace slampp

#include "preload.h"
SLAMPP_PRELOAD_UNIT(dense_tiles) // (the handle's bring-up thread loads this unit's code object: capi.hip)
