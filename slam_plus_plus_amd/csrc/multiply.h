// multiply.h -- y = alpha Lambda x + beta y on the caller's block structure, and the fixed-order reductions that go with it
// (multiply.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

namespace slampp {

// A block row with more blocks than this (its column's own blocks plus the blocks of its row list) is cut into chunks;
// a chunk holds at most multiply_CHUNK blocks (SLAMPP_HIP_MULTIPLY_* in include/slampp_hip.h: the tests name them)
enum { multiply_LONG_ROW = 256, multiply_CHUNK = 256, multiply_MAX_UNROLLED_DIM = 8, reduce_MAX_PARTIALS = 1024 };

struct CMultiplyState;

// host lists of the structure (one thread: two passes over the blocks, 2 ms at 10^6 of them) and their upload; n_long_row:
// the split threshold in use (multiply_LONG_ROW, or what the development option "multiply_long_row" says).  Throws.
CMultiplyState *multiply_setup(int64_t n_bcols, const std::vector<int64_t> &r_cumsum, const std::vector<int64_t> &r_bcol_ptr,
	const std::vector<int32_t> &r_brow, int n_long_row, hipStream_t stream);
void multiply_destroy(CMultiplyState *p);
size_t multiply_device_bytes(const CMultiplyState *p);
int multiply_long_row_threshold(const CMultiplyState *p);
// enqueue-only; beta = 0: y is not read
void multiply_enqueue(const CMultiplyState &r_state, const double *p_values, const double *p_x, double *p_y, double f_alpha,
	double f_beta, hipStream_t stream);

// *p_out = sum a_i b_i / max |a_i| over n entries in two passes: at most reduce_MAX_PARTIALS workgroups whose number depends on n
// alone, each summing a fixed set of entries in a fixed tree, then one workgroup over their partial results in index order.
// p_partials: reduce_MAX_PARTIALS doubles of workspace
void dot_enqueue(const double *p_a, const double *p_b, int64_t n, double *p_partials, double *p_out, hipStream_t stream);
void norm_inf_enqueue(const double *p_a, int64_t n, double *p_partials, double *p_out, hipStream_t stream);

// one step of iterative refinement around the re-solve: keep = x and x += d (nothing added once *p_stop is set); then, with
// the residual norm *p_trial of the new x, the step stands if 2 *p_trial <= *p_prev, and otherwise x = keep and *p_stop = 1.
// *p_next: the norm of the x that is left.  p_next differs from p_prev and p_trial.
enum { refine_MAX_STEPS = 8, refine_TRIAL = refine_MAX_STEPS + 1, refine_STOP, refine_SCALARS }; // (the scalars of one call)
void refine_step_enqueue(double *p_x, double *p_keep, const double *p_d, int64_t n, const double *p_stop, hipStream_t stream);
void refine_accept_enqueue(double *p_x, const double *p_keep, int64_t n, const double *p_prev, const double *p_trial,
	double *p_next, double *p_stop, hipStream_t stream);

} // namespace slampp
