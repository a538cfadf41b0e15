// oracle/tile_probe.cpp -- test infrastructure (tests/test_dense_tiles_gpu.py), not the product: one C entry point that
// runs the dense top's two schedules (csrc/dense_chol.h, nothing else of the library) on a matrix and a tile pattern handed
// in directly, and hands back every intermediate result and the device tables of the tile schedule.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>
#include "dense_chol.h"

using namespace slampp;

namespace {

struct TDevice { // frees what the call allocated on every way out
	std::vector<void*> ptrs;
	hipStream_t stream = 0;
	~TDevice()
	{
		for(size_t i = 0; i < ptrs.size(); ++ i)
			(void)hipFree(ptrs[i]);
		if(stream)
			(void)hipStreamDestroy(stream);
	}
	template <class T> T *Alloc(size_t n, hipError_t &r_err)
	{
		void *p = 0;
		if(r_err == hipSuccess && (r_err = hipMalloc(&p, std::max(n, size_t(1)) * sizeof(T))) == hipSuccess)
			ptrs.push_back(p);
		return (T*)p;
	}
};

#define PROBE_CHECK(x) do { hipError_t e_ = (x); if(e_ != hipSuccess) { (void)hipGetLastError(); return int(e_); } } while(0)

} // anonymous namespace

// T, p_nonzero: the tile pattern (T * T flags, column-major); n: the system's size, n_pad = 64 T >= n + 1 (more than a tile of padding is allowed);
// p_matrix: n_pad x n_pad, column-major, lower triangle, the right-hand side in row n_pad - 1, padding diagonal set;
// p_rhs_again: n entries, the second right-hand side.
// Out: p_L_tile, p_L_dense (n_pad x n_pad each): the matrix after tile_cholesky (and the second forward substitution's y in
// its last row) and after dense_cholesky; p_x (3 n_pad): the solutions of tile_cholesky + tile_backsolve, of
// dense_forwardsolve + tile_backsolve with the second right-hand side, of dense_cholesky + dense_backsolve;
// p_status: {flag of the tile schedule, flag of the dense schedule, Build's return value, n_levels};
// p_table_size (14) and p_tables (n_table_capacity ints): the device tables copied back, then the host pointer arrays,
// in the order potrf, trsm, tgt, src, riders, back_diag, back_carry, level_potrf_ptr, level_trsm_ptr, level_tgt_ptr,
// level_urgent_end, rider_ptr, back_diag_ptr, back_carry_ptr (sizes in ints).
// Returns 0, a HIP error code, or -1 for arguments it cannot take, -2 where the tables do not fit.
extern "C" int tile_probe_run(int T, const char *p_nonzero, int n, const double *p_matrix, const double *p_rhs_again,
	double *p_L_tile, double *p_L_dense, double *p_x, int *p_status, int *p_table_size, int *p_tables, int n_table_capacity)
{
	if(T <= 0 || T > 64 || n < 1 || n + 1 > T * dense_NB)
		return -1;
	const int n_pad = T * dense_NB;
	const size_t n_elems = size_t(n_pad) * n_pad, n_bytes = n_elems * sizeof(double);
	TDevice dev;
	PROBE_CHECK(hipStreamCreate(&dev.stream));
	hipStream_t stream = dev.stream;
	hipError_t e = hipSuccess;
	double *d_M = dev.Alloc<double>(n_elems, e), *d_invdiag = dev.Alloc<double>(size_t(T) * dense_NB * dense_NB, e),
		*d_z = dev.Alloc<double>(n_pad, e), *d_x = dev.Alloc<double>(n_pad, e);
	int *d_flag = dev.Alloc<int>(2, e);
	PROBE_CHECK(e);
	PROBE_CHECK(hipMemsetAsync(d_flag, 0, 2 * sizeof(int), stream));
	std::fill(p_status, p_status + 4, 0);
	std::fill(p_table_size, p_table_size + 14, 0);
	std::fill(p_x, p_x + 3 * size_t(n_pad), 0.0);

	// the tile schedule: factor and solve, then another right-hand side on the kept factor
	{
		CTileSchedule schedule;
		const bool b_built = schedule.Build(T, std::vector<char>(p_nonzero, p_nonzero + size_t(T) * T), stream);
		p_status[2] = int(b_built);
		p_status[3] = schedule.n_levels;
		if(b_built) {
			PROBE_CHECK(hipMemcpyAsync(d_M, p_matrix, n_bytes, hipMemcpyHostToDevice, stream));
			PROBE_CHECK(hipMemsetAsync(d_z, 0, n_pad * sizeof(double), stream));
			PROBE_CHECK(hipMemsetAsync(d_x, 0, n_pad * sizeof(double), stream));
			tile_cholesky(schedule, d_M, n_pad, n, d_invdiag, d_flag, stream);
			tile_backsolve(schedule, d_M, n_pad, n, d_invdiag, d_z, d_x, stream);
			PROBE_CHECK(hipGetLastError());
			PROBE_CHECK(hipMemcpyAsync(p_x, d_x, n_pad * sizeof(double), hipMemcpyDeviceToHost, stream));
			PROBE_CHECK(hipMemcpy2DAsync(d_M + (n_pad - 1), size_t(n_pad) * sizeof(double), p_rhs_again, sizeof(double),
				sizeof(double), n, hipMemcpyHostToDevice, stream)); // into the last row, columns < n
			dense_forwardsolve(d_M, n_pad, d_invdiag, stream);
			tile_backsolve(schedule, d_M, n_pad, n, d_invdiag, d_z, d_x, stream);
			PROBE_CHECK(hipGetLastError());
			PROBE_CHECK(hipMemcpyAsync(p_x + n_pad, d_x, n_pad * sizeof(double), hipMemcpyDeviceToHost, stream));
			PROBE_CHECK(hipMemcpyAsync(p_L_tile, d_M, n_bytes, hipMemcpyDeviceToHost, stream));
			PROBE_CHECK(hipStreamSynchronize(stream));
			// the tables as the device holds them
			const int n_potrf = schedule.level_potrf_ptr.back(), n_trsm = schedule.level_trsm_ptr.back(),
				n_tgt = schedule.level_tgt_ptr.back(), n_riders = schedule.rider_ptr.back(),
				n_diag = schedule.back_diag_ptr.back(), n_carry = schedule.back_carry_ptr.back();
			std::vector<int4> tgt(n_tgt), riders(n_riders);
			if(n_tgt)
				PROBE_CHECK(hipMemcpy(tgt.data(), schedule.d_tgt, n_tgt * sizeof(int4), hipMemcpyDeviceToHost));
			if(n_riders)
				PROBE_CHECK(hipMemcpy(riders.data(), schedule.d_riders, n_riders * sizeof(int4), hipMemcpyDeviceToHost));
			int n_src = 0; // (the schedule does not keep the length of its source list: as far as a record points)
			for(int i = 0; i < n_tgt; ++ i)
				n_src = std::max(n_src, tgt[i].w);
			for(int i = 0; i < n_riders; ++ i)
				n_src = std::max(n_src, riders[i].w);
			const void *p_dev[7] = {schedule.d_potrf, schedule.d_trsm, schedule.d_tgt, schedule.d_src, schedule.d_riders,
				schedule.d_back_diag, schedule.d_back_carry};
			const int p_dev_size[7] = {n_potrf, 4 * n_trsm, 4 * n_tgt, n_src, 4 * n_riders, 4 * n_diag, 4 * n_carry};
			const std::vector<int> *p_host[7] = {&schedule.level_potrf_ptr, &schedule.level_trsm_ptr, &schedule.level_tgt_ptr,
				&schedule.level_urgent_end, &schedule.rider_ptr, &schedule.back_diag_ptr, &schedule.back_carry_ptr};
			size_t n_total = 0;
			for(int i = 0; i < 7; ++ i)
				n_total += size_t(p_dev_size[i]) + p_host[i]->size();
			if(n_total > size_t(std::max(n_table_capacity, 0)))
				return -2;
			int *p_out = p_tables;
			for(int i = 0; i < 7; ++ i) {
				if(p_dev_size[i])
					PROBE_CHECK(hipMemcpy(p_out, p_dev[i], p_dev_size[i] * sizeof(int), hipMemcpyDeviceToHost));
				p_table_size[i] = p_dev_size[i];
				p_out += p_dev_size[i];
			}
			for(int i = 0; i < 7; ++ i) {
				std::copy(p_host[i]->begin(), p_host[i]->end(), p_out);
				p_table_size[7 + i] = int(p_host[i]->size());
				p_out += p_host[i]->size();
			}
		}
	}

	// the dense schedule on a fresh copy
	PROBE_CHECK(hipMemcpyAsync(d_M, p_matrix, n_bytes, hipMemcpyHostToDevice, stream));
	PROBE_CHECK(hipMemsetAsync(d_z, 0, n_pad * sizeof(double), stream));
	PROBE_CHECK(hipMemsetAsync(d_x, 0, n_pad * sizeof(double), stream));
	dense_cholesky(d_M, n_pad, n, d_invdiag, d_flag + 1, stream);
	dense_backsolve(d_M, n_pad, n, d_invdiag, d_z, d_x, stream);
	PROBE_CHECK(hipGetLastError());
	PROBE_CHECK(hipMemcpyAsync(p_x + 2 * size_t(n_pad), d_x, n_pad * sizeof(double), hipMemcpyDeviceToHost, stream));
	PROBE_CHECK(hipMemcpyAsync(p_L_dense, d_M, n_bytes, hipMemcpyDeviceToHost, stream));
	PROBE_CHECK(hipMemcpyAsync(p_status, d_flag, 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
	PROBE_CHECK(hipStreamSynchronize(stream));
	return 0;
}
