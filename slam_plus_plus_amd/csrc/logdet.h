// logdet.h -- log det of a factored matrix from the pivots of its Cholesky factor (logdet.hip; slampp_hip_logdet)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace slampp {

// what the lanes of the first pass read: three kinds of items, any of which may be absent (count 0)
struct TLogdetSources {
	// pivots listed by a table (logdet_tables.h): entry >= 0 an offset into p_L, entry < 0 position -(1 + entry) on the
	// diagonal of the dense top p_dense (leading dimension n_dense_ld)
	const int64_t *p_table;
	int64_t n_table;
	const double *p_L, *p_dense;
	int64_t n_dense_ld;
	// the first n_diag diagonal entries of a dense factor (the reduced camera system after dense_cholesky)
	const double *p_diag;
	int64_t n_diag, n_diag_ld;
	// the landmarks of a Schur-mode system (block sizes n_dc, n_dp): their diagonal blocks C_p are read from the packed
	// values and factored in registers; p_ptr: the block column pointers of Lambda, n_cams block columns come first
	const double *p_values;
	const int64_t *p_ptr;
	int64_t n_cams, n_points;
	int n_dc, n_dp;
};

// *p_out = 2 sum log(pivot) over all items, or NaN if *p_flag is set (p_flag may be null).  Two launches whose shape depends
// on the number of items alone, no atomics: the same call gives the same bits.  p_partials: reduce_MAX_PARTIALS doubles.
void logdet_enqueue(const TLogdetSources &r_src, double *p_partials, const int *p_flag, double *p_out, hipStream_t stream);

} // namespace slampp
