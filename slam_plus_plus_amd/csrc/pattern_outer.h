// pattern_outer.h -- the symmetric outer product of two vectors on Lambda's block pattern, the adjoint of
// y = alpha Lambda x + beta y with respect to the packed values (pattern_outer.hip; its host tables: pattern_outer_tables.h)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

namespace slampp {

struct CPatternOuterState;

// host tables of the structure (one thread, one pass over the blocks) and their upload.  Throws.
CPatternOuterState *pattern_outer_setup(int64_t n_bcols, const std::vector<int64_t> &r_cumsum, const std::vector<int64_t> &r_bcol_ptr,
	const std::vector<int32_t> &r_brow, hipStream_t stream);
void pattern_outer_destroy(CPatternOuterState *p);
size_t pattern_outer_device_bytes(const CPatternOuterState *p);
// enqueue-only, one launch for the n_batch members (member m: p_a + m n_a_stride, p_b + m n_b_stride, p_out + m n_out_stride);
// beta = 0: out is not read
void pattern_outer_enqueue(const CPatternOuterState &r_state, int n_batch, const double *p_a, int64_t n_a_stride, const double *p_b,
	int64_t n_b_stride, double *p_out, int64_t n_out_stride, double f_alpha, double f_beta, hipStream_t stream);
// out = alpha sum over k < n_terms of P(a_k, b_k) + beta out (a_k = p_a + k n_a_stride, b_k = p_b + k n_b_stride), one launch
// that writes out once; the terms are added in ascending k, one term gives the bits of pattern_outer_enqueue
void pattern_outer_sum_enqueue(const CPatternOuterState &r_state, int n_terms, const double *p_a, int64_t n_a_stride, const double *p_b,
	int64_t n_b_stride, double *p_out, double f_alpha, double f_beta, hipStream_t stream);

} // namespace slampp
