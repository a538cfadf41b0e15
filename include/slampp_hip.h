/*
 * slampp_hip.h -- C ABI of libslampp_hip.so: an MI355X (gfx950) sparse block Cholesky /
 * Schur-complement solver for the normal equations  Lambda * dx = eta  of SLAM++.
 *
 * This is the drop-in boundary for the reference's linear-solver concept
 * (/root/reference/include/slam/LinearSolverTags.h:38-135).  The reference binds its solvers
 * as compile-time template parameters, so the binding a maintainer adds is the header class
 * include/slam/LinearSolver_HIP.h (CLinearSolver_HIP / CLinearSolver_Schur_HIP), which gathers
 * the blocks of a CUberBlockMatrix and forwards to the entry points below.  Each entry point
 * names the reference call it stands in for.
 *
 * Conventions
 *   - plain C types only; all functions return a status (SLAMPP_HIP_*), never throw, never exit;
 *   - Lambda is passed exactly as the reference stores it (BlockMatrixBase.h:380-503): block-CSC,
 *     only the upper triangle populated (LinearSolver_CholMod.cpp:57), block rows sorted inside a
 *     block column, each block dense column-major;  values are passed packed in that block order;
 *   - eta is overwritten with the solution (same contract as Solve_PosDef, LinearSolver_CholMod.h:186);
 *   - a handle is not thread-safe; different handles are independent (no process-global state).
 */
#ifndef SLAMPP_HIP_H_INCLUDED
#define SLAMPP_HIP_H_INCLUDED

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slampp_hip_solver slampp_hip_solver; /* opaque */

enum {
	SLAMPP_HIP_OK = 0,
	SLAMPP_HIP_NOT_POSDEF = 1,          /* reference: Solve_PosDef returns false (LinearSolver_CholMod.cpp:310-317) */
	SLAMPP_HIP_ERR_INVALID = -1,        /* bad argument / call order */
	SLAMPP_HIP_ERR_ALLOC = -2,          /* host or device out of memory (reference: std::bad_alloc) */
	SLAMPP_HIP_ERR_DEVICE = -3,         /* HIP runtime error (reference: std::runtime_error, LinearSolver_Schur.h:1196-1209) */
	SLAMPP_HIP_ERR_UNSUPPORTED = -4     /* an operation outside what this build handles for this structure (block columns wider than 8 are cut into pieces at analysis time and solved; see slampp_hip_factorize / slampp_hip_marginals for what they still need) */
};

enum {
	SLAMPP_HIP_MODE_SPARSE = 0,         /* pose-graph path: fill-reducing ordering + sparse block Cholesky */
	SLAMPP_HIP_MODE_SCHUR = 1           /* BA path: Schur complement on the last (landmark) block columns, dense reduced system */
};

/* phase wall-clock of the last factor_solve, ms; names follow the reference's timers
 * (NonlinearSolver_Lambda.h:250, LinearSolver_Schur.h:1896-1911) */
typedef struct slampp_hip_times {
	double order_ms, symbolic_ms, upload_ms, factor_ms, solve_ms, download_ms;  /* sparse path */
	double schur_ms, reduce_ms, cholsol_ms, backsubst_ms;                        /* Schur path */
	double total_ms;
} slampp_hip_times;

typedef struct slampp_hip_stats {
	int64_t n_bcols, n_blocks_upper, n_scalars, nnz_upper;  /* Lambda, as given */
	int64_t l_blocks, l_nnz;          /* block / scalar nonzeros of the factor under our ordering */
	double  factor_flops, solve_flops; /* CHOLMOD's convention: sum of squared column counts; 4*lnz */
	int64_t n_stages, n_tasks, etree_height, n_update_pairs;
	int64_t n_cams, n_points, n_observations, schur_dim;     /* Schur path, else 0 (sparse path: schur_dim = dimension of the dense top) */
	int64_t device_bytes;
	int64_t n_bottom_stages;          /* leading (wide) stages: stage 0 by the lane-per-task kernel, the others one wave per task */
} slampp_hip_stats;

/* lifecycle -- stands in for the solver object's ctor / dtor / Free_Memory()
 * (LinearSolver_CholMod.h:148-167).  device_id: HIP device ordinal.
 * SLAMPP_HIP_ERR_DEVICE without a usable device of that ordinal (there is no CPU fallback).  The handle's HIP streams are
 * created on a thread of the library's while the caller goes on to set_structure / analyze (milliseconds each in a process
 * that has made none yet); the first entry point that needs them waits for that thread and is the one to report
 * SLAMPP_HIP_ERR_DEVICE if they could not be made. */
int slampp_hip_create(slampp_hip_solver **pp_solver, int device_id);

/* One handle over several devices of this process (SURVEY.md section 8b proposed create(device_ids*, n_dev); section 8e:
 * BA shards by landmark).  The reference's nonlinear solvers call their linear solver from one thread of one process
 * (include/slam/NonlinearSolver_Base.h:344-346,400,438; NonlinearSolver_Lambda_LM.h:1543-1552), so this is how a BA
 * solve reaches GPUs 1..n-1 behind the unchanged CLinearSolver_* calls: in SCHUR mode slampp_hip_analyze cuts the
 * landmarks into n contiguous shards balanced by observation count (slampp_hip_landmark_shard), every device gets an
 * internal solver and a host thread of its own, slampp_hip_factor_solve / _schur_marginals / _solve_marginal_poses send
 * each member its landmark columns of Lambda straight from the caller's (pinned) arrays over its own PCIe link, the
 * partial reduced camera systems are summed by an all-reduce inside the library -- RCCL bound at run time (dlopen of
 * librccl.so, ncclCommInitAll over the device list, rings over xGMI), or a direct exchange through peer pointers where
 * RCCL is absent or a device is listed twice (option "group_exchange": 0 = that choice, 1 = RCCL or fail, 2 = peer
 * pointers; environment SLAMPP_HIP_GROUP_EXCHANGE=rccl|peer) -- and every member writes its landmarks' part of the
 * solution into the caller's vector.  In SPARSE mode (pose graphs: one elimination tree, nothing to shard) the handle
 * is a plain solver on p_device_ids[0].  n_devices = 1 is slampp_hip_create.  The entry points that take device
 * pointers (…_device, …_device_async, slampp_hip_sync) apply to one device and return SLAMPP_HIP_ERR_INVALID on a
 * handle that is solving with shards; slampp_hip_set_allreduce likewise (the exchange is the library's).  A device may
 * be listed more than once (that is how the 1-GPU test boxes run two members). */
int slampp_hip_create_multi(slampp_hip_solver **pp_solver, const int *p_device_ids, int n_devices);

/* what a handle made by slampp_hip_create_multi is doing: members in use (0 = not sharded: one device, sparse mode, or
 * not analyzed yet), the landmark range [p_point_bounds[r], p_point_bounds[r + 1]) of every member (n + 1 entries, may
 * be NULL) and the exchange in use ("rccl (<library>)" / "peer" / "none"; valid until the next analyze) */
int slampp_hip_group_info(const slampp_hip_solver *p_solver, int *p_member_num, int64_t *p_point_bounds, int n_max_members,
	const char **pp_s_exchange);

/* how many exchanges (all-reduces of the reduced camera system) the members of a device group have gone into since the
 * handle was made.  Failure agreement: before a collective is enqueued the members meet at a host barrier with their
 * status, for RCCL and peer pointers alike; when one of them failed on its way there (allocation, upload, device error)
 * NOBODY enqueues -- the call returns that member's error, this count does not move, the next solve runs normally.  The
 * option "group_fail_member" = r + 1 makes member r fail that way (0 = off; a test hook).  The reference has no
 * counterpart: it is one thread on one device (include/slam/NonlinearSolver_Lambda_LM.h:1543-1552). */
int slampp_hip_group_exchange_count(const slampp_hip_solver *p_solver, int64_t *p_n_enqueued);

/* the exchange of slampp_hip_create_multi by itself, for deployment checks and tests: one member per listed device,
 * every member fills n_count doubles with a pattern of its own, the buffers are summed twice through the members'
 * all-reduce (n_exchange as the option "group_exchange": 0 / 1 = RCCL / 2 = peer pointers; 1 also runs with a single
 * device: the RCCL calls themselves) and every member checks every entry.  p_s_exchange_out receives the name of the
 * exchange used (or what went wrong). */
int slampp_hip_group_exchange_selftest(const int *p_device_ids, int n_devices, int n_exchange, int64_t n_count,
	char *p_s_exchange_out, int n_max_chars);

/* the landmark shard a rank of a multi-GPU BA solve holds, host code only (no GPU, no handle): rank n_rank of n_world
 * keeps block columns [0, n_matrix_cut) -- the cameras -- and a contiguous range of the landmark block columns balanced
 * by observation count; first call with the three pointers NULL for the sizes.  The shard's packed values are values
 * [0, n_camera_values) followed by values [n_value_begin, n_value_end) of the full system, its right-hand side entries
 * [0, n_camera_scalars) followed by [n_scalar_begin, n_scalar_end); the camera blocks and the camera part of eta are
 * added by one rank only (option "shard_primary").  The same rule as slam_plus_plus_amd/sharding.py. */
typedef struct slampp_hip_shard_view {
	int64_t n_bcols, n_blocks;
	int64_t n_camera_values, n_value_begin, n_value_end;
	int64_t n_camera_scalars, n_scalar_begin, n_scalar_end;
	int64_t n_point_begin, n_point_end;
	int64_t *p_bcol_cumsum;   /* [n_bcols + 1] */
	int64_t *p_bcol_ptr;      /* [n_bcols + 1] */
	int32_t *p_brow_idx;      /* [n_blocks] */
} slampp_hip_shard_view;
int slampp_hip_landmark_shard(int64_t n_bcols, const int64_t *p_bcol_cumsum, const int64_t *p_bcol_ptr,
	const int32_t *p_brow_idx, int64_t n_matrix_cut, int n_rank, int n_world, slampp_hip_shard_view *p_view);

void slampp_hip_destroy(slampp_hip_solver *p_solver);
int slampp_hip_free_memory(slampp_hip_solver *p_solver);
const char *slampp_hip_last_error(const slampp_hip_solver *p_solver);

/* Options (20).  All but the ones marked (*) take effect at the next slampp_hip_analyze.
 *
 * ordering / schedule of the sparse block path
 *   "natural_order"      0 / 1: keep the caller's block order instead of nested dissection (default 0; what
 *                        Factorize_PosDef_Blocky needs: the reference factors the matrix as it is ordered)
 *   "leaf_size"          nested-dissection leaf, in block columns (default 3)
 *   "subtree_size"       most columns one wave eliminates sequentially at the bottom of the tree (default 8)
 *   "task_height"        1 .. 8 (default 6): above the wide stages a separator task is a slice of the elimination tree this
 *                        many levels high; a launch covers that many levels, the slice's blocks stay in LDS
 *   "dense_top_nb"       block columns with at least this many blocks, and their ancestors, are factored as one dense matrix on
 *                        the matrix cores (default 24, or 16 / 36 where a model of the dependent launch chain prefers that;
 *                        setting the option fixes the threshold; 0 = off)
 *   "dense_top_max_dim"  cap on its dimension (default 12288)
 *   "dense_top_min_dim"  below this dimension there is no dense top (default 192)
 * Schur mode
 *   "schur_sparse"       how the reduced camera system S is factored: -1 (default) = by the sparse block path when fewer than
 *                        15 % of its camera-camera blocks are nonzero, 0 = dense on the matrix cores, 1 = sparse (the reference
 *                        chooses at compile time: __SCHUR_USE_DENSE_SOLVER, include/slam/LinearSolver_Schur.h:48-55)
 *   "schur_tiles"        how S = A - U C^-1 U^T is assembled: -1 (default) = landmark by landmark (runs of landmarks seen by the
 *                        same cameras on the matrix cores, tiles of neighbouring landmarks in LDS) where that takes at least
 *                        half of the contributions, per-block contribution lists for the rest; 0 = lists only; 1 / 2 / 3 =
 *                        runs and tiles wherever possible / tiles only / runs of any length
 *   "schur_incremental"  0 / 1 / 2: keep the assembled S for slampp_hip_schur_set_changed_points; 1 = a solve with a list of
 *                        changed landmarks updates it when that is the shorter way, 2 = whenever a list is given
 *   "schur_keep"         0 (default) / 1: every solve also stores W = U C^-1 and leaves the factor of S valid for another
 *                        right-hand side (slampp_hip_solve_again, slampp_hip_solve_again_device_async, slampp_hip_refine)
 *   "schur_fallback"     default 1: a structure the Schur kernels do not take (no landmark part, landmark-landmark blocks,
 *                        block sizes other than (6,3), (7,3), (3,2)) is solved by the sparse block path, as the reference
 *                        solves it (LinearSolver_Schur.h:1635-1638, 1721-1726); 0 = slampp_hip_analyze reports
 *                        SLAMPP_HIP_ERR_UNSUPPORTED / _INVALID instead
 *   "marginals_dense"    (*) 1 = slampp_hip_schur_marginals always inverts S densely; 0 (default) = a sparse inverse subset on
 *                        the factor's pattern when the solves factor S by the sparse block path
 * several GPUs
 *   "shard_primary"      process-per-GPU sharding: this rank adds A and eta_x (default 1)
 *   "shard_rank", "shard_world"  (*) optional: who this rank is among the ranks behind the all-reduce callback; lets them
 *                        exchange their block lists instead of an indicator over all camera pairs (limited to 16384 cameras)
 *   "group_exchange"     handles made by slampp_hip_create_multi, see there
 * host side
 *   "staging_ahead"      (*) 0 / 1: slampp_hip_analyze also brings up the pinned host staging of slampp_hip_host_staging on a
 *                        thread of its own next to the ordering (callers that hand over host arrays: the header class sets it)
 *   "assembly_groups"    (*) slampp_hip_assembly_create: the most vertices one group of the Lambda assembly takes (default: as
 *                        many as fit in LDS; 0 = no groups, one wave per block of Lambda)
 *   "profile"            (*) 0 / 1 / 2 / 3, see slampp_hip_get_profile
 *
 * Anything else set_option knows ("panel", "panel_rows", "panel_handup", "panel_backward", "simt", "simt_width", "simt_stages",
 * "simt_backward", "wide_min_tasks", "nd_balance", "dense_nb", "dense_top_tiles", "schur_distributed", "group_fail_member", "multiply_long_row")
 * is a development option: an alternative the defaults were measured against, or a test hook.  They are refused with
 * SLAMPP_HIP_ERR_INVALID unless the process runs with SLAMPP_HIP_DEV=1, and are described where they are implemented
 * (csrc/solver.h). */
int slampp_hip_set_option(slampp_hip_solver *p_solver, const char *p_s_name, int64_t n_value);

/* structure of Lambda -- stands in for what the reference's wrappers read through
 * n_BlockColumn_Num() / n_BlockColumn_Base() / n_BlockColumn_Block_Num() / n_Block_Row()
 * (BlockMatrix.h:343-392,407-431) and for p_BlockStructure_to_Sparse (BlockMatrix.cpp:3880-3958).
 * Calling it again means "the block structure changed" = Clear_SymbolicDecomposition()
 * (LinearSolverTags.h:112-120). */
int slampp_hip_set_structure(slampp_hip_solver *p_solver, int64_t n_bcols,
	const int64_t *p_bcol_cumsum /* [n_bcols+1] */, const int64_t *p_bcol_ptr /* [n_bcols+1] */,
	const int32_t *p_brow_idx /* [n_blocks] */);

/* ordering + symbolic analysis -- stands in for SymbolicDecomposition_Blocky()
 * (LinearSolver_CholMod.cpp:868-951, LinearSolver_UberBlock.h:256-310; Schur: LinearSolver_Schur.h:1566-1606).
 * SCHUR mode: block columns [n_matrix_cut, n_bcols) are the landmarks (the reference's guided
 * ordering, LinearSolver_Schur.cpp:771-838, puts them last); they must form a block-diagonal C. */
int slampp_hip_analyze(slampp_hip_solver *p_solver, int n_mode, int64_t n_matrix_cut);

/* numeric factorization + solve -- stands in for Solve_PosDef_Blocky(lambda, eta)
 * (LinearSolverTags.h:130-134; LinearSolver_CholMod.cpp:738-866; LinearSolver_Schur.h:1623-1935).
 * p_values: packed block values of Lambda (host); p_rhs_inout: eta on entry, dx on return (host).
 * Returns SLAMPP_HIP_NOT_POSDEF if a pivot is not positive. p_times may be NULL. */
int slampp_hip_factor_solve(slampp_hip_solver *p_solver, const double *p_values,
	double *p_rhs_inout, slampp_hip_times *p_times);

/* Pinned host staging owned by the library, for callers that have to gather Lambda's values anyway (the header class:
 * a CUberBlockMatrix keeps its blocks in pooled pages behind per-block pointers, BlockMatrixBase.h:321,374,449-453):
 * *pp_values receives room for the packed values, *pp_rhs for the right-hand side / solution (either may be NULL).
 * Passing exactly these pointers to slampp_hip_factor_solve / _factorize / _marginals / _schur_marginals /
 * _solve_marginal_poses makes the transfers single DMA copies without a staging pass; any other host array is moved
 * through the same staging in chunks (1 MB first, doubling up to 32 MB) by a few host threads while the previous chunk is on the bus.  Valid until
 * the next slampp_hip_set_structure / _free_memory / _destroy (call again after set_structure). */
int slampp_hip_host_staging(slampp_hip_solver *p_solver, double **pp_values, double **pp_rhs);

/* Sends values [n_first, n_first + n_count) of the staging on their way (a copy stream of the library's own) while
 * the caller is still gathering the rest: chunks must follow each other, n_first = 0 starts a new pass; the next call
 * that takes the staged values sends what is left and waits for all of it.  Enqueue-only. */
int slampp_hip_upload_values_async(slampp_hip_solver *p_solver, int64_t n_first, int64_t n_count);

/* same with both arrays already resident in device memory (HBM); used by bench.py so that the
 * timed region excludes PCIe.  p_rhs_inout_dev is overwritten with the solution. */
int slampp_hip_factor_solve_device(slampp_hip_solver *p_solver, const double *p_values_dev,
	double *p_rhs_inout_dev, slampp_hip_times *p_times);

/* another right-hand side with the factor of the last factor_solve
 * (reference: cholmod_solve / cs_lsolve+cs_ltsolve on a kept factor, LinearSolver_CholMod.cpp:322-347) */
int slampp_hip_solve_again(slampp_hip_solver *p_solver, double *p_rhs_inout);

/* ... and the same with the vector resident in device memory, enqueue-only on the solver's stream, in both modes.
 * Sparse mode: the two substitutions with the kept factor; SLAMPP_HIP_ERR_INVALID without one (nothing factored yet, a
 * factorization that was not positive definite, a batch that went through the handle's factor arrays).
 * Schur mode: a BA solve keeps the factor of the reduced camera system S and C^-1, and with the option "schur_keep" (or
 * "schur_incremental") also W = U C^-1; the re-solve is CHOLMOD's kept-factor solve inside the reference's Schur steps
 * (LinearSolver_CholMod.cpp:322-347 within LinearSolver_Schur.h:1830-1886), without reading Lambda's values again:
 *   r = eta_c - sum_p W_p eta_p   (per camera over its observations, fixed order),   S dx = r   (the dense factor's or the
 *   inner sparse solver's substitutions),   dl_p = C_p^-1 eta_p - sum over the cameras c of p of W_(c,p)^T dx_c.
 * Valid after a solve with "schur_keep" = 1 or "schur_incremental" >= 1 that was positive definite, or after
 * slampp_hip_schur_marginals_pattern / _schur_marginal_columns (which leave W, C^-1 and the factor of S -- or, where they
 * inverted the dense S in place of its factor, that inverse, which is then multiplied with); anything that factors, or fails
 * to, since (another solve without the option, slampp_hip_schur_marginals, marginal poses, a batch, set_structure, analyze, a
 * slampp_hip_sync that reports SLAMPP_HIP_NOT_POSDEF) ends it: SLAMPP_HIP_ERR_INVALID, and slampp_hip_last_error names the
 * option.  Landmark shards (an all-reduce callback, a handle over several devices): SLAMPP_HIP_ERR_UNSUPPORTED.  A Schur
 * handle whose analysis went to the sparse path ("schur_fallback") answers as the sparse path does.
 * The host slampp_hip_solve_again takes the same route in Schur mode when such a factor is valid; without one it answers as
 * before (SLAMPP_HIP_ERR_UNSUPPORTED after a plain Schur solve). */
int slampp_hip_solve_again_device_async(slampp_hip_solver *p_solver, double *p_rhs_inout_dev);

/* n_columns right-hand sides with the kept factor in one call -- cholmod_solve with a dense B of several columns, which the
 * reference's linear solvers sit on (LinearSolver_CholMod.cpp:322-347): J Sigma J^T, Lambda^-1 B, several adjoints of one
 * backward pass, block Krylov and sampling code, LM steps at several damped right-hand sides.  Column c is the n_scalars doubles at
 * p_rhs_inout_dev + c * n_ld, in the caller's scalar order: eta on entry, Lambda^-1 eta on return; the n_ld - n_scalars
 * doubles behind a column are not touched.  Valid exactly when slampp_hip_solve_again_device_async is, in both modes, with
 * its error codes and its slampp_hip_last_error texts under the name solve_columns (landmark shards:
 * SLAMPP_HIP_ERR_UNSUPPORTED).  SLAMPP_HIP_ERR_INVALID: a null pointer, n_columns outside 1 .. SLAMPP_HIP_SOLVE_MAX_COLUMNS,
 * n_ld < n_scalars with more than one column.
 * Sparse mode, block columns of at most 8: both substitutions run on all the columns at once, over the static plan of the
 * single-vector substitutions, one launch per stage and pass of at most 48 columns; a lane owns one (row of a block,
 * right-hand side) pair, so a wave carries 64 / d right-hand sides (10 at 6 x 6 blocks) and every block of L is read once
 * for them; the permutation to and from the caller's order is fused into the kernels.  With a dense top its columns'
 * reduced right-hand sides go through k-column tile solves on the top's factor.  The factor is read once per pass and
 * group of right-hand sides, where n_columns calls of slampp_hip_solve_again_device_async read it n_columns times.  Measured
 * on 100 000 SE(3) poses: 8 columns in the time of 1.8 single re-solves, 48 in the time of 6.5; 2
 * columns win 10 % only, and one column is better served by slampp_hip_solve_again_device_async (the call's launches are
 * latency-bound up to the right-hand sides of one wave).  The results agree with slampp_hip_solve_again_device_async to
 * rounding, not to the bit (another summation order).
 * Schur mode, and sparse mode with block columns wider than 8 (factored in pieces): no k-column kernels here (W and the
 * factor are read once per column) -- the call runs the single-vector route of slampp_hip_solve_again_device_async column
 * by column, from either kept state, and gives its bits.
 * No atomics.  Column c's result depends on column c alone: not on n_columns, not on its place, and a NaN in one column
 * reaches no other.  The same call twice gives the same bits.  Enqueue-only on the handle's stream, but for the first call
 * after an analysis, which builds the row lists of the dense-top columns on the host and waits for their upload.
 * Installs no factor.  slampp_hip_solve_columns: host array (column-major, leading dimension n_ld), through device memory
 * in groups of 48 columns; it waits. */
#define SLAMPP_HIP_SOLVE_MAX_COLUMNS 256
int slampp_hip_solve_columns_device_async(slampp_hip_solver *p_solver, double *p_rhs_inout_dev, int64_t n_ld, int n_columns);
int slampp_hip_solve_columns(slampp_hip_solver *p_solver, double *p_rhs_inout, int64_t n_ld, int n_columns);

/* The two substitutions of the call above one at a time: y = L^-1 P b and x = P^T L^-T y -- cholmod_solve with CHOLMOD_P +
 * CHOLMOD_L and with CHOLMOD_Lt + CHOLMOD_Pt, and what the reference's L / FastL solvers are built on:
 * UpperTriangularTranspose_Solve_FBS gives d = R^-T eta and UpperTriangular_Solve_FBS gives dx = R^-1 d, each on its own
 * (include/slam/NonlinearSolver_FastL.h:1101, 1693, 2305-2406, NonlinearSolver_L.h:941-1136, 2254-2458,
 * BlockMatrix.h:3284-3580).  With the forward half alone: b^T Lambda^-1 b = |L^-1 P b|^2 (the chi^2 of a candidate loop
 * closure, the Newton decrement eta^T Lambda^-1 eta), whitened residuals, and B Lambda^-1 B^T = Y^T Y for k linear
 * functionals (slampp_hip_gram_device_async below); with the backward half alone: samples x = P^T L^-T z of covariance
 * Lambda^-1 from standard normal z.
 * Columns as in slampp_hip_solve_columns: column c is the n_scalars doubles at p_inout_dev + c * n_ld, 1 <= n_columns <=
 * SLAMPP_HIP_SOLVE_MAX_COLUMNS, the n_ld - n_scalars doubles behind a column are not touched, n_ld is not read for one column.
 *   SLAMPP_HIP_HALF_FORWARD:  b in the caller's scalar order on entry, y = L^-1 P b in the factor's order on return;
 *   SLAMPP_HIP_HALF_BACKWARD: y in the factor's order on entry, x = P^T L^-T y in the caller's scalar order on return.
 * The factor's order: new block j is the caller's block perm[j] of slampp_hip_factor_structure, its dim[j] scalars next to
 * each other, the blocks one after the other (j ascending); L is the factor slampp_hip_factorize hands back for the same
 * values, so L L^T = P Lambda P^T in that order.
 * Valid when slampp_hip_solve_again_device_async is valid in sparse mode (a Schur handle whose analysis went to the sparse
 * path included), with its SLAMPP_HIP_ERR_INVALID and texts under the name solve_half_columns; SLAMPP_HIP_ERR_INVALID also
 * for another n_half, a null pointer, n_columns out of range, n_ld < n_scalars with more than one column.
 * SLAMPP_HIP_ERR_UNSUPPORTED, slampp_hip_last_error saying why: Schur mode (the factor there is the block factor
 * [L_S, U L_C^-T; 0, L_C]; its halves need L_C of every landmark, where the handle keeps C^-1), block columns wider than 8
 * (factored in pieces), landmark shards.
 * The launches are those of slampp_hip_solve_columns_device_async in its order, in passes of 48 columns, cut in two between
 * the substitutions; the forward half then copies y out of the interleaved workspace into the caller's columns (a dense
 * top's rows out of the tile solves' array), the backward half first copies it in -- transposes through an LDS tile, whole
 * lines on both sides.  (The forward kernels cannot write y into the caller's array themselves: they still read b there, in
 * the caller's order, while other tasks write y in the factor's.)  So a forward call followed by a backward call on its
 * result gives the bits of slampp_hip_solve_columns_device_async, with or without a dense top.  No atomics; column c depends
 * on column c alone (a NaN stays in its column); the same call twice gives the same bits; installs no factor.  Enqueue-only
 * but for the first call after an analysis (the host-side lists of slampp_hip_solve_columns).
 * slampp_hip_solve_half_columns: host array, through device memory in groups of 48 columns; it waits. */
#define SLAMPP_HIP_HALF_FORWARD  0
#define SLAMPP_HIP_HALF_BACKWARD 1
int slampp_hip_solve_half_columns_device_async(slampp_hip_solver *p_solver, int n_half, double *p_inout_dev, int64_t n_ld,
	int n_columns);
int slampp_hip_solve_half_columns(slampp_hip_solver *p_solver, int n_half, double *p_inout, int64_t n_ld, int n_columns);

/* y = alpha Lambda x + beta y with Lambda's packed values as slampp_hip_factor_solve_device reads them -- what the
 * reference's LM and dog-leg solvers compute on the host after every linear solve: the gain ratio's dx^T (alpha dx + eta)
 * and the Cauchy step's g^T Lambda g (include/slam/NonlinearSolver_Lambda_LM.h:207, NonlinearSolver_Lambda_DL.h:1175-1177 and 1270:
 * CUberBlockMatrix::PostMultiply_Add and PreMultiply_Add on the upper triangle).  Lambda is the symmetric matrix whose
 * upper blocks are stored: a stored block (r, c), r < c, contributes B x_c to y_r and B^T x_r to y_c; diagonal blocks are read
 * as the full d x d blocks the solver reads.  Needs slampp_hip_set_structure only (no analysis, either mode); the caller's
 * structure is used as given, block columns wider than 8 go through a generic (slow) kernel.  No atomics: every entry of y is
 * summed in a fixed order (ascending block column; rows with more than SLAMPP_HIP_MULTIPLY_LONG_ROW blocks in chunks of
 * SLAMPP_HIP_MULTIPLY_CHUNK whose partial sums are added in chunk order), two calls give the same bits.  beta = 0 does not
 * read y (it may hold NaN).  x == y: SLAMPP_HIP_ERR_INVALID; a handle solving with landmark shards: SLAMPP_HIP_ERR_UNSUPPORTED.
 * Enqueue-only on the solver's stream, but for the first call after a set_structure: that one builds the row lists on the
 * host and, where lists of an earlier structure exist, waits for the stream before it frees them.  The lists live until
 * the next set_structure (slampp_hip_analyze leaves them; slampp_hip_free_memory frees them).
 * slampp_hip_multiply: host arrays, the values through the staging of slampp_hip_host_staging. */
#define SLAMPP_HIP_MULTIPLY_LONG_ROW 256
#define SLAMPP_HIP_MULTIPLY_CHUNK 256
int slampp_hip_multiply_device_async(slampp_hip_solver *p_solver, const double *p_values_dev, const double *p_x_dev,
	double *p_y_dev, double f_alpha, double f_beta);
int slampp_hip_multiply(slampp_hip_solver *p_solver, const double *p_values, const double *p_x, double *p_y,
	double f_alpha, double f_beta);

/* out = alpha P(a, b) + beta out on Lambda's block pattern, where P(a, b) is the adjoint of the product above with respect to
 * the packed values: <v, P(a, b)> = a^T M(v) b for the symmetric M(v) that slampp_hip_multiply defines from the values v.
 * It is what the gradient of a solve needs (x = M(v)^-1 eta and an upstream gradient x_bar: g = M^-1 x_bar on the kept
 * factor, eta_bar = g, v_bar = -P(g, x)), and what a Gauss-Newton caller that differentiates through Lambda would form:
 *   out(r, c) = alpha (a_r b_c^T + b_r a_c^T) + beta out(r, c)   for every stored block with r < c,
 *   out(r, r) = alpha  a_r b_r^T              + beta out(r, r)   for every diagonal block (the full d x d block);
 * out has the length and the layout of p_values (same block order, blocks column-major).  Needs slampp_hip_set_structure only
 * (no analysis, either mode, any block dimensions).  No atomics and no reductions: every value is at most two products and one
 * add in one fixed form, so two calls give the same bits, batched or not.  beta = 0 does not read out (it may hold NaN).
 * The kernel is a stream over the packed array: a thread owns pairs of consecutive values and writes each with one 16-byte
 * store (a pair may lie in two blocks); a member whose out is not 16-byte aligned is written with 8-byte stores, to the same bits.
 * SLAMPP_HIP_ERR_INVALID: a null pointer, no structure, n_batch outside 1 .. SLAMPP_HIP_MAX_BATCH, a stride below the length
 * of one member (n_scalars for a and b, the number of values for out; the strides of a batch of one are not read), out
 * overlapping a or b (a == b is fine).  A handle solving with landmark shards: SLAMPP_HIP_ERR_UNSUPPORTED.
 * Enqueue-only on the solver's stream, but for the first call after a set_structure: that one builds lookup tables on the
 * host (per block: its offset and the scalar rows it pairs; per 128 values: their first block) and, where tables of an earlier
 * structure exist, waits for the stream before it frees them.  The tables live as the product's row lists do: until the
 * next set_structure (slampp_hip_analyze leaves them; slampp_hip_free_memory frees them).
 * _batch_: member m reads p_a_dev + m n_a_stride and p_b_dev + m n_b_stride and writes p_out_values_dev + m n_out_stride
 * (strides in doubles), one launch for all members.  slampp_hip_pattern_outer: host arrays. */
int slampp_hip_pattern_outer_device_async(slampp_hip_solver *p_solver, const double *p_a_dev, const double *p_b_dev,
	double *p_out_values_dev, double f_alpha, double f_beta);
int slampp_hip_pattern_outer(slampp_hip_solver *p_solver, const double *p_a, const double *p_b, double *p_out_values,
	double f_alpha, double f_beta);
int slampp_hip_pattern_outer_batch_device_async(slampp_hip_solver *p_solver, int n_batch, const double *p_a_dev,
	int64_t n_a_stride, const double *p_b_dev, int64_t n_b_stride, double *p_out_values_dev, int64_t n_out_stride,
	double f_alpha, double f_beta);

/* out = alpha sum over k < n_terms of P(a_k, b_k) + beta out, a_k = p_a_dev + k n_a_stride, b_k = p_b_dev + k n_b_stride
 * (strides in doubles), P as above: the adjoint of a k-column solve with respect to the values (x_k = M^-1 eta_k and upstream
 * gradients: g = slampp_hip_solve_columns of them, v_bar = -sum P(g_k, x_k)).  The same streaming kernel: a thread keeps its
 * pair of values in registers over the terms, adds them in ascending k in one fixed form and writes out once; beta = 0 does
 * not read out.  One term gives the bits of slampp_hip_pattern_outer_device_async; two calls give the same bits, whatever
 * the alignment of out (16-byte stores where it is 16-byte aligned, 8-byte stores otherwise).  The checks of the batched call:
 * SLAMPP_HIP_ERR_INVALID for a null pointer, no structure, n_terms outside 1 .. SLAMPP_HIP_SOLVE_MAX_COLUMNS, a stride below
 * n_scalars (not read for one term), out overlapping any a_k or b_k; landmark shards: SLAMPP_HIP_ERR_UNSUPPORTED.
 * Enqueue-only as the calls above. */
int slampp_hip_pattern_outer_sum_device_async(slampp_hip_solver *p_solver, int n_terms, const double *p_a_dev, int64_t n_a_stride,
	const double *p_b_dev, int64_t n_b_stride, double *p_out_values_dev, double f_alpha, double f_beta);

/* *p_out_dev = sum a_i b_i over n device-resident entries, in two passes of a fixed shape (it depends on n alone): bit-
 * reproducible like the product.  With it the scalars of the LM / dog-leg step control (Eigen's dot products in
 * NonlinearSolver_Lambda_LM.h:207, NonlinearSolver_Lambda_DL.h:1270, 1510) stay on the device.  Enqueue-only; any handle. */
int slampp_hip_dot_device_async(slampp_hip_solver *p_solver, const double *p_a_dev, const double *p_b_dev, int64_t n,
	double *p_out_dev);

/* The same grown to a block: out(i, j) = sum over r < n_rows of a_i[r] b_j[r], a_i = p_a_dev + i * n_lda (i < n_ka), b_j =
 * p_b_dev + j * n_ldb (j < n_kb), out(i, j) = p_out_dev[i + j * n_ldo] -- n_ka x n_kb, column-major; 1 <= n_ka, n_kb <=
 * SLAMPP_HIP_GRAM_MAX_COLUMNS.  With a == b == Y, the columns slampp_hip_solve_half_columns_device_async left of B^T, it is the
 * Gram matrix Y^T Y = B Lambda^-1 B^T (Eigen's products around the triangular solves in the reference's L solvers,
 * NonlinearSolver_FastL.h:2305-2406).  Two launches whose shape depends on n_rows, n_ka and n_kb alone: the rows in chunks of
 * 2 048 (longer ones, in whole tiles of 64 rows, once that would be more than 256 chunks), a workgroup per chunk that stages
 * 64 rows of both operands in LDS at a time and sums its partial block on the matrix cores (v_mfma_f64_16x16x4: four rows to
 * an instruction, the rows in order, four row groups added in a fixed order); then the partial blocks are added in chunk order.  No atomics: two calls give the same bits, and
 * with a == b out(i, j) and out(j, i) have the same bits.  The partial blocks live in a workspace of 256 x 48 x 48 doubles
 * (4.5 MiB) that the first call allocates.  Any handle, no structure or factor needed; enqueue-only.  SLAMPP_HIP_ERR_INVALID:
 * a null pointer, n_rows < 0, n_ka or n_kb out of range, n_lda or n_ldb below n_rows (not read for one column), n_ldo < n_ka,
 * out overlapping a or b; landmark shards: SLAMPP_HIP_ERR_UNSUPPORTED, as slampp_hip_dot_device_async. */
#define SLAMPP_HIP_GRAM_MAX_COLUMNS 48
#define SLAMPP_HIP_GRAM_CHUNK_ROWS 2048
int slampp_hip_gram_device_async(slampp_hip_solver *p_solver, const double *p_a_dev, int64_t n_lda, int n_ka,
	const double *p_b_dev, int64_t n_ldb, int n_kb, int64_t n_rows, double *p_out_dev, int64_t n_ldo);

/* Iterative refinement of a solution x of Lambda x = eta with the kept factor: n_steps (1 .. 8) times r = eta - Lambda x,
 * d = solve_again(r), x += d -- the classical loop around cholmod_solve (LinearSolver_CholMod.cpp:322-347; the reference
 * itself does not refine).  A step stands only if it at least halves max |eta - Lambda x| (the test LAPACK's xPORFS
 * continues on: below that the fp64 residual is its own rounding noise); otherwise x is put back as it was and the steps
 * after it change nothing, so the call never returns an x with a larger residual norm than it was given.  All of it is
 * decided on the device.  p_resid_inf_dev (n_steps + 1 doubles, or NULL): entry k = max |eta - Lambda x_k| of the x held
 * before step k, the last one that of the x returned (a fixed-order max; the entries never grow).  Needs what
 * slampp_hip_solve_again_device_async needs (SLAMPP_HIP_ERR_INVALID otherwise) and the values the factor was made of; one
 * workspace of 2 n_scalars doubles (the residual and the x to go back to), allocated once; enqueue-only.  The residual is
 * computed in plain fp64 (with fused multiply-adds), not in extended precision: the steps lower the backward error of x
 * towards that of the residual's own rounding, they do not promise a smaller forward error where cond(Lambda) * eps is
 * near 1.  slampp_hip_refine: host arrays. */
int slampp_hip_refine_device_async(slampp_hip_solver *p_solver, const double *p_values_dev, const double *p_eta_dev,
	double *p_x_inout_dev, int n_steps, double *p_resid_inf_dev);
int slampp_hip_refine(slampp_hip_solver *p_solver, const double *p_values, const double *p_eta, double *p_x_inout, int n_steps,
	double *p_resid_inf);

/* log det M(v) = 2 sum log L_ii from the Cholesky factor on the device, one double (M(v): the symmetric matrix
 * slampp_hip_multiply defines) -- what CHOLMOD users sum from the factor's diagonal: the Gaussian log-likelihood and Laplace
 * evidence of a graph, D-optimality, information gain.  In Schur mode log det Lambda = log det S + sum_p log det C_p: the
 * pivots of the reduced camera system's factor, and every landmark's block C_p read from the values and factored in
 * registers (not taken from the stored C_p^-1, whose determinant loses accuracy with cond(C_p)^2).
 * b_reuse_factor = 0: the values (required) are factored first -- numeric factorization only in sparse mode without a dense
 * top; with a dense top, and in Schur mode, a solve on a zero right-hand side of the library's own -- and the handle is left
 * exactly as slampp_hip_factor_solve_device_async of these values leaves it (slampp_hip_solve_again*, the covariance calls
 * with values = NULL, "schur_keep" / "schur_incremental" by the rules they state).
 * b_reuse_factor = 1: nothing is factored, the factor in place is read.  Sparse mode: valid exactly when
 * slampp_hip_solve_again_device_async is; the values are not read and may be NULL.  Schur mode: valid exactly while a solve
 * that kept its factor (option "schur_keep" or "schur_incremental") is the handle's latest factorization; the values are
 * required (the landmark term is computed from them) and trusted to be the ones the factor was made of, as slampp_hip_refine
 * trusts its values.  What a Schur covariance call left does not serve: its dense route holds inv(L), not L.  No valid
 * factor: SLAMPP_HIP_ERR_INVALID, with the reason in slampp_hip_last_error, before anything is enqueued.
 * Two launches whose shape depends on the number of pivots alone, no atomics: the same call gives the same bits.  If the
 * handle's not-positive-definite flag is raised when the second launch runs, NaN is written (decided on the device), and
 * slampp_hip_sync reports SLAMPP_HIP_NOT_POSDEF as for any factorization.  Enqueue-only on the handle's stream; the table
 * of the pivots' places is built on the host at the first call after an analysis.  slampp_hip_logdet: host arrays; it waits,
 * returns SLAMPP_HIP_NOT_POSDEF and leaves NaN in *p_logdet where the matrix is not positive definite.
 * SLAMPP_HIP_ERR_UNSUPPORTED for a handle that solves with landmark shards (an all-reduce callback, a device group);
 * SLAMPP_HIP_ERR_INVALID for a null output, or null values where they are required.  A Schur-mode handle whose analysis
 * went to the sparse path answers as the sparse path does. */
int slampp_hip_logdet_device_async(slampp_hip_solver *p_solver, const double *p_values_dev, int b_reuse_factor,
	double *p_logdet_dev);
int slampp_hip_logdet(slampp_hip_solver *p_solver, const double *p_values, int b_reuse_factor, double *p_logdet);

/* Numeric factorization only, the factor handed back to the host -- for CLinearSolverTag-style callers that keep
 * the factor themselves (the reference's Factorize_PosDef_Blocky, LinearSolver_CholMod.cpp:362-544, used by its
 * L / FastL solvers on a matrix they have ordered: set the option "natural_order" to 1 for that).  p_factor_out
 * receives l_values doubles: the lower factor L of the permuted Lambda, block-CSC over the CALLER's block columns as
 * slampp_hip_factor_structure describes it (perm, dim, lptr / lrow / loff), blocks column-major, the diagonal block
 * first in each column.  Like the reference's it takes any matrix: big separators are factored as one dense matrix on
 * the matrix cores (the "dense top") and their columns handed back in the same block layout; block columns wider than
 * 8 are factored in pieces and put together again (those only in the caller's own order: natural_order = 1).
 * Returns SLAMPP_HIP_NOT_POSDEF if a pivot is not positive. */
int slampp_hip_factorize(slampp_hip_solver *p_solver, const double *p_values, double *p_factor_out);
/* ... and the block structure of that factor (after slampp_hip_analyze, sparse mode): sizes through the first three
 * pointers, arrays where the pointers are not NULL -- perm[new] = old and dim[new] over the caller's n_bcols block
 * columns, lptr [n_bcols + 1], lrow / loff [l_blocks].  Stands in for the structure the reference's factor comes back
 * in, a CUberBlockMatrix (LinearSolver_CholMod.cpp:520-544: From_Sparse into r_factor). */
int slampp_hip_factor_structure(const slampp_hip_solver *p_solver, int64_t *p_n_bcols, int64_t *p_l_blocks, int64_t *p_l_values,
	int32_t *p_perm, int32_t *p_dim, int64_t *p_lptr, int32_t *p_lrow, int64_t *p_loff);

/* Schur mode, option "schur_incremental" = 1 (set before slampp_hip_analyze): the next factor_solve updates the reduced
 * camera system the previous factor_solve of this handle assembled instead of rebuilding it -- the reference's dog-leg
 * solver does the same from Omega = Lambda_new - Lambda_old (include/slam/NonlinearSolver_Lambda_DL.h:1025-1086, 2301-).
 * p_points (host): the landmarks, as indices among the landmark block columns, strictly increasing, whose blocks (C_p and
 * the U blocks of their observations) differ from the previous call's values; the camera-camera blocks and the
 * right-hand side may differ freely; n_points = 0 says that no landmark changed.  The contributions of the named
 * landmarks are exchanged (the old ones rebuilt from W = U C^-1 and C^-1, which the previous solve left on the device)
 * with fp64 atomic adds, so this path -- unlike every other one -- does not sum in a fixed order.  One-shot; falls back
 * to the full rebuild when there is nothing valid to update (first solve, a solve that was not positive definite, a
 * covariance call in between, landmark shards).  With the option on, the dense reduced system is kept in a second
 * n_pad^2 buffer (the factorization works in place). */
int slampp_hip_schur_set_changed_points(slampp_hip_solver *p_solver, const int64_t *p_points, int64_t n_points);

/* Schur mode only: solves for the landmarks alone, dl = C^-1 eta_l, and zeroes the camera part of the vector -- the
 * reference's CLinearSolver_Schur::Solve_PosDef_Blocky_MarginalPoses (include/slam/LinearSolver_Schur.h:1956-2143).
 * Returns SLAMPP_HIP_NOT_POSDEF if a landmark block is not positive definite (the reference inverts it regardless). */
int slampp_hip_solve_marginal_poses(slampp_hip_solver *p_solver, const double *p_values, double *p_rhs_inout);
int slampp_hip_solve_marginal_poses_device_async(slampp_hip_solver *p_solver, const double *p_values_dev,
	double *p_rhs_inout_dev);

/* Sparse mode: block diagonal of the covariance matrix Lambda^-1 -- what the reference's nonlinear solvers get from
 * CMarginals::Calculate_DenseMarginals_Recurrent_FBS(margs, R, ordering, mpart_Diagonal) after ordering and factoring
 * Lambda once more on the host for the purpose (include/slam/NonlinearSolver_Lambda.h:700-760, "todo - reuse what the
 * linear solver calculated").  Numeric factorization, then the blocks of the inverse on the factor's pattern by the
 * recursion run from the root of the elimination tree downwards; p_block_diag receives one dim x dim column-major block
 * per block column, in the order of slampp_hip_set_structure.  Where the plan has a dense top, its part of the
 * inverse is the dense inverse of the top's Schur complement (matrix cores), and the recursion continues below it.
 * One block size (3, 6 or 7: unrolled kernels), or -- like the reference's, Marginals.h:1694, which takes any -- a mix of
 * block sizes up to 8 (poses and landmarks in one graph): block c is d_c x d_c, the blocks follow each other; that
 * one without a dense top (option dense_top_nb = 0).  Block columns wider than 8: SLAMPP_HIP_ERR_UNSUPPORTED. */
int slampp_hip_marginals(slampp_hip_solver *p_solver, const double *p_values, double *p_block_diag);
int slampp_hip_marginals_device_async(slampp_hip_solver *p_solver, const double *p_values_dev, double *p_block_diag_dev);

/* Sparse mode: Lambda^-1 at every stored block of Lambda -- the reference's CMarginals::Calculate_DenseMarginals_Recurrent_FBS
 * computes the inverse on the pattern of its factor R (include/slam/Marginals.h:1696, b_structure_of_R); R's pattern
 * depends on the ordering, so ours and CHOLMOD's differ, while Lambda's pattern is the same for every ordering and lies
 * inside every factor's pattern: that is the pattern returned here.  p_cov has the length and layout of p_values (same
 * block order, each block d_r x d_c column-major), so a caller can wrap it in Lambda's block structure.  Numeric
 * factorization and the sparse inverse subset as slampp_hip_marginals, then one gather of the upper blocks (block (r, c)
 * is read as the stored block (max, min) of the permuted pair, transposed where the permutation flips the pair; pairs
 * inside the dense top element-wise from its dense inverse).  Same inputs as slampp_hip_marginals; Schur mode, handles
 * over several devices and block columns wider than 8: SLAMPP_HIP_ERR_UNSUPPORTED.  Leaves the factor in place
 * (slampp_hip_solve_again, slampp_hip_marginal_columns with values = NULL). */
int slampp_hip_marginals_pattern(slampp_hip_solver *p_solver, const double *p_values, double *p_cov);
int slampp_hip_marginals_pattern_device_async(slampp_hip_solver *p_solver, const double *p_values_dev, double *p_cov_dev);

/* Sparse mode: whole block columns of Lambda^-1 -- the reference's mpart_Column / mpart_LastColumn parts
 * (include/slam/IncrementalPolicy.h:366-372, computed by CMarginals::Calculate_DenseMarginals_Recurrent_FBS from
 * NonlinearSolver_Lambda.h:690-752 after ordering and factoring Lambda once more, the last vertex kept last).
 * p_bcols (host): n_cols distinct block column indices; p_out: n_scalars x k doubles, column-major, k = the sum of the
 * listed columns' dimensions, in the listed order; rows in the caller's scalar order.  p_values = NULL: the factor in
 * place from the last factor_solve, marginals, marginals_pattern or marginal_columns call is used (SLAMPP_HIP_ERR_INVALID
 * without one, e.g. after a factorization that was not positive definite, or a batch); otherwise these values are
 * factored first.  Multi-right-hand-side substitutions with that factor, in passes of at most 48 scalar columns (a
 * device workspace of n_scalars x 48 doubles, allocated once): the forward one only over the listed columns' paths to
 * the root of the elimination tree, the backward one over every column.  n_cols <= 0, an index out of range or listed
 * twice: SLAMPP_HIP_ERR_INVALID; Schur mode, several devices, block columns wider than 8: SLAMPP_HIP_ERR_UNSUPPORTED.
 * Returns SLAMPP_HIP_NOT_POSDEF as the solve does.  The host version brings the result back in groups of at most 48
 * columns (the device holds n_scalars x 48 of it at a time). */
int slampp_hip_marginal_columns(slampp_hip_solver *p_solver, const double *p_values, int n_cols, const int64_t *p_bcols,
	double *p_out);
int slampp_hip_marginal_columns_device_async(slampp_hip_solver *p_solver, const double *p_values_dev, int n_cols,
	const int64_t *p_bcols, double *p_out_dev);

/* Sparse mode: blocks of Lambda^-1 at arbitrary pairs of block columns -- what a front end asks for when it gates loop
 * closures or tests joint compatibility (Sigma_ii, Sigma_jj, Sigma_ij of candidate pairs that are not edges yet; g2o's
 * computeMarginals(spinv, blockIndices), GTSAM's jointMarginalCovariance).  p_brows, p_bcols (host): n_pairs block column
 * indices each; pair k gives the d_r x d_c block Lambda^-1[rows of block column p_brows[k], columns of block column
 * p_bcols[k]], column-major, and the blocks follow each other in p_out in the listed order.  With Lambda = P^T L L^T P,
 *   Lambda^-1(r, c) = (L^-1 P E_r)^T (L^-1 P E_c) = Y_r^T Y_c,
 * and Y_j is nonzero only on the path of j to the root of the elimination tree: the pruned forward substitution of
 * slampp_hip_marginal_columns gives all of it, in passes of at most 48 scalar right-hand sides (both columns of a pair in one
 * pass, pairs taken in the listed order until the next would not fit); there is no backward substitution and no
 * n_scalars x k result.  A Gram kernel then sums, per pair, over the rows both paths share -- from their lowest common
 * ancestor to the root, the dense top included -- in a fixed order without atomics: the same call gives the same bits.
 * Nothing is refused about the pairs themselves: r < c, r > c (the block as it stands in the symmetric inverse) and r == c,
 * inside Lambda's pattern or outside it, a column in any number of pairs, a pair listed twice (each listing is computed).
 * p_values = NULL: the factor in place, by the rule of slampp_hip_marginal_columns (SLAMPP_HIP_ERR_INVALID without one);
 * otherwise these values are factored first and the factor stays in place.  n_pairs <= 0, a null pointer, an index out of
 * range: SLAMPP_HIP_ERR_INVALID; Schur mode, several devices, landmark shards, block columns wider than 8:
 * SLAMPP_HIP_ERR_UNSUPPORTED (a Schur handle whose analysis went to the sparse path answers).  Returns
 * SLAMPP_HIP_NOT_POSDEF as the solve does, and leaves no factor then.  The device version only enqueues, once its lists
 * are built on the host; the host version brings the blocks back in one copy. */
int slampp_hip_marginal_blocks(slampp_hip_solver *p_solver, const double *p_values, int64_t n_pairs, const int64_t *p_brows,
	const int64_t *p_bcols, double *p_out);
int slampp_hip_marginal_blocks_device_async(slampp_hip_solver *p_solver, const double *p_values_dev, int64_t n_pairs,
	const int64_t *p_brows, const int64_t *p_bcols, double *p_out_dev);

/* Schur mode only: block diagonal of the covariance matrix Lambda^-1 -- the reference's
 * CSchurComplement_Marginals::Schur_Marginals (include/slam/BAMarginals.h:579-806, called from
 * NonlinearSolver_Lambda_LM.h:1326 and NonlinearSolver_Lambda_DL.h:1640 with the Cholesky factor of the Schur
 * complement it has to compute for the purpose).  Here the reduced camera system is assembled, factored and inverted
 * on the device in one call: p_cam_cov receives n_cams blocks of dc x dc doubles (the diagonal blocks of S^-1; may be
 * NULL to skip them, as b_do_cam_marginals = false does), p_point_cov n_points blocks of dp x dp doubles
 * (C_p^-1 + W_p^T S^-1 W_p), column-major, in the block order of slampp_hip_set_structure.  When the solves
 * factor the reduced system by the sparse block path (option "schur_sparse"), the blocks of S^-1 come from a sparse
 * inverse subset on that factor's pattern (every camera pair that shares a landmark is in it); otherwise, or with
 * option "marginals_dense", S is inverted densely (2 x 8 n^2 bytes of device memory, n = n_cams dc).  With landmark
 * shards every rank calls it, passes its own values and receives the covariances of its own landmarks (the
 * all-reduce callback is invoked once, on the packed blocks or on the whole n_pad^2 buffer).  Returns
 * SLAMPP_HIP_NOT_POSDEF like the solve. */
int slampp_hip_schur_marginals(slampp_hip_solver *p_solver, const double *p_values, double *p_cam_cov, double *p_point_cov);
int slampp_hip_schur_marginals_device_async(slampp_hip_solver *p_solver, const double *p_values_dev,
	double *p_cam_cov_dev, double *p_point_cov_dev);

/* Schur mode: covariances beyond the block diagonal of a BA system.  The reference has none: after its Schur marginals
 * (NonlinearSolver_Lambda_LM.h:1362, "could use fast Schur marginals but at the moment those only implement recovery of
 * mpart_Diagonal") it orders and factors the whole of Lambda on the host and runs the recursive formula.  Here, with
 * Lambda = [A U; U^T C], S = A - U C^-1 U^T, Z = S^-1, W_o = U_o C_p^-1:
 *   camera blocks (a, b)     Z(a, b)
 *   observation (c, p)       -sum over the cameras b observing p of Z(c, b) W_b
 *   landmark p               C_p^-1 + W_p^T Z W_p
 * slampp_hip_schur_marginals_pattern: p_cov has the length and layout of p_values and receives Lambda^-1 at every stored
 * (upper) block -- camera blocks of A, every observation block (dc x dp), every landmark diagonal block -- each column-major.
 * Its diagonal blocks are those of slampp_hip_schur_marginals.  Z comes from the dense inverse of S or from the sparse
 * inverse subset on its factor, decided as slampp_hip_schur_marginals decides (options "schur_sparse", "marginals_dense").
 * slampp_hip_schur_marginal_columns: whole block columns, cameras or landmarks in any mix, laid out as by
 * slampp_hip_marginal_columns (n_scalars x k, column-major, listed order).  A camera column is Z E_c on the cameras and
 * -W_p^T Z(cams(p), c) on every landmark p; a landmark column is -Z W E_p on the cameras, then the same per landmark plus
 * C_p^-1 on its own block.  Passes of at most 48 scalar columns: the camera part is gathered from the dense inverse of S, or
 * solved by multi-right-hand-side substitutions with S's sparse factor; the landmark rows follow per landmark.
 * p_values = NULL (either call): the factor of S, C^-1 and W left by the previous call of these two (or of
 * slampp_hip_schur_marginal_blocks) on this handle are
 * used; SLAMPP_HIP_ERR_INVALID if any other factorization ran since (a solve, schur_marginals, marginal poses, a batch) or if
 * that one was not positive definite.  Both calls recompute C^-1 and W from the values given: a later incremental solve
 * (slampp_hip_schur_set_changed_points) rebuilds the reduced system.  A handle whose Schur analysis went to the sparse
 * path (option "schur_fallback") answers as slampp_hip_marginals_pattern / slampp_hip_marginal_columns (same layouts).
 * Sparse mode, several devices, landmark shards: SLAMPP_HIP_ERR_UNSUPPORTED.  Bad column lists: SLAMPP_HIP_ERR_INVALID.
 * Returns SLAMPP_HIP_NOT_POSDEF as the solve does. */
int slampp_hip_schur_marginals_pattern(slampp_hip_solver *p_solver, const double *p_values, double *p_cov);
int slampp_hip_schur_marginals_pattern_device_async(slampp_hip_solver *p_solver, const double *p_values_dev, double *p_cov_dev);
int slampp_hip_schur_marginal_columns(slampp_hip_solver *p_solver, const double *p_values, int n_cols, const int64_t *p_bcols,
	double *p_out);
int slampp_hip_schur_marginal_columns_device_async(slampp_hip_solver *p_solver, const double *p_values_dev, int n_cols,
	const int64_t *p_bcols, double *p_out_dev);

/* Schur mode: blocks of Lambda^-1 of a BA system at arbitrary pairs of block columns, in the layout of
 * slampp_hip_marginal_blocks: the indices are block columns of slampp_hip_set_structure (cameras < n_matrix_cut, landmarks
 * after), pair k gives the d_r x d_c block, column-major, and the blocks follow each other in p_out in the listed order.  The
 * joint covariance of two cameras that share no landmark, of two landmarks, of a camera and a landmark it does not observe
 * yet: none of these is in Lambda's pattern, and slampp_hip_schur_marginal_columns would form n_scalars x k doubles to read
 * a few small blocks out of them.  With Lambda^-1 = [Z, -Z W; -W^T Z, C^-1 + W^T Z W] (the notation above):
 *   camera a, camera b        Z(a, b)
 *   camera a, landmark q      -sum over b in cams(q) of Z(a, b) W_{b,q}
 *   landmark p, camera b      the transpose of the above
 *   landmark p, landmark q    delta_pq C_p^-1 + sum over a in cams(p), b in cams(q) of W_{a,p}^T Z(a, b) W_{b,q}
 * Two routes, decided as slampp_hip_schur_marginals decides (options "schur_sparse", "marginals_dense").  S inverted densely:
 * one workgroup per pair sums its block from the dense inverse, its lanes striding over the camera pairs (a, b), the partial
 * sums meeting by lane shuffles and LDS in a fixed order.  S factored by the sparse block path, S = P^T L L^T P: with
 * Y_c = L^-1 P E_c for a camera column and Y_q = L^-1 P (-W E_q) for a landmark column all four cases are
 *   Lambda^-1(r, c) = Y_r^T Y_c   (+ C_p^-1 when r = c = landmark p),
 * Y nonzero on the union of the elimination-tree paths of the cameras behind the column: passes of at most 48 scalar
 * right-hand sides (both columns of a pair in one pass, pairs taken in the listed order until the next would not fit), each
 * the pruned forward substitution and a Gram kernel over the rows two such unions share; no backward substitution, no
 * inverse of S, no n_scalars x k result.  Neither route uses atomics: the same call gives the same bits.
 * Nothing is refused about the pairs themselves: r < c, r > c and r == c, cameras and landmarks in any mix, inside Lambda's
 * pattern or outside it, a column in any number of pairs, a pair listed twice (each listing is computed); a pair and its
 * twin (c, r) are exact transposes of each other.
 * p_values = NULL: the factor of S (or its dense inverse), C^-1 and W left by the previous call of the Schur covariance
 * family on this handle (slampp_hip_schur_marginals_pattern, _schur_marginal_columns or this one) are used,
 * SLAMPP_HIP_ERR_INVALID under the conditions of slampp_hip_schur_marginal_columns; otherwise the values are factored first.
 * The call leaves all of that in place: the other two calls with p_values = NULL and slampp_hip_solve_again_device_async are
 * valid afterwards by the rules they state.  n_pairs <= 0, a null pointer, an index out of range: SLAMPP_HIP_ERR_INVALID,
 * decided before anything is enqueued.  Sparse mode (use slampp_hip_marginal_blocks), several devices, landmark shards:
 * SLAMPP_HIP_ERR_UNSUPPORTED.  A handle whose Schur analysis went to the sparse path (option "schur_fallback") answers as
 * slampp_hip_marginal_blocks (same layout).  Returns SLAMPP_HIP_NOT_POSDEF as the solve does, and leaves nothing to reuse
 * then.  The device version only enqueues, once its lists are built on the host; the host version brings the blocks back
 * in one copy. */
int slampp_hip_schur_marginal_blocks(slampp_hip_solver *p_solver, const double *p_values, int64_t n_pairs, const int64_t *p_brows,
	const int64_t *p_bcols, double *p_out);
int slampp_hip_schur_marginal_blocks_device_async(slampp_hip_solver *p_solver, const double *p_values_dev, int64_t n_pairs,
	const int64_t *p_brows, const int64_t *p_bcols, double *p_out_dev);

/* enqueue-only variants for benchmarking / stream capture: no host synchronisation, no status
 * read-back; slampp_hip_sync() waits and returns OK / NOT_POSDEF / error for everything enqueued since the
 * previous slampp_hip_sync() (NOT_POSDEF if any of those factorizations was not positive definite) */
int slampp_hip_factor_solve_device_async(slampp_hip_solver *p_solver, const double *p_values_dev,
	double *p_rhs_inout_dev);
int slampp_hip_sync(slampp_hip_solver *p_solver);

/* K value sets of the analyzed structure in ONE pass of launches -- K damping values of one Lambda, K graphs of one shape --,
 * sparse mode: member k reads p_values_dev + k * n_values_stride and overwrites p_rhs_inout_dev + k * n_rhs_stride with its
 * solution (strides in doubles, at least the length of one member's array; 16-byte aligned bases and even strides let the
 * members share launches, anything else is solved one member after the other with the same result).  The chain of dependent
 * launches is as long as for one system and every launch K times as wide: a pose-graph solve fills a fraction of the
 * chip, K of them fill it.  Stands where the reference's LM loop re-damps and re-solves one value after the other
 * (NonlinearSolver_Lambda_LM.h:967-1001, 1660-1676); SURVEY section 8(e): pose graphs do not shard, "replicas only
 * (multiple independent problems / damping values per GPU)".  slampp_hip_sync_batch waits and reports per member:
 * p_status[k] = SLAMPP_HIP_OK or SLAMPP_HIP_NOT_POSDEF (a member that is not positive definite does not disturb the
 * others).  The handle's own factor (slampp_hip_solve_again, covariances) is not touched by a batch of more than one that
 * shares launches.  A batch that is solved member by member (a dense top, regrouped block columns, unaligned bases or odd
 * strides) goes through the handle's factor arrays: after more than one such member the handle has NO factor of its own
 * (slampp_hip_solve_again and the covariance calls return SLAMPP_HIP_ERR_INVALID until the next factorization); a batch of
 * one is an ordinary factorization, and its factor is dropped if slampp_hip_sync_batch reports the member not positive definite. */
#define SLAMPP_HIP_MAX_BATCH 64
int slampp_hip_factor_solve_batch_device_async(slampp_hip_solver *p_solver, int n_batch, const double *p_values_dev,
	int64_t n_values_stride, double *p_rhs_inout_dev, int64_t n_rhs_stride);
int slampp_hip_sync_batch(slampp_hip_solver *p_solver, int *p_status /* [n_batch] */, int n_batch);
void *slampp_hip_stream(slampp_hip_solver *p_solver); /* the hipStream_t every kernel is launched on */

int slampp_hip_get_stats(const slampp_hip_solver *p_solver, slampp_hip_stats *p_stats);

/* Schur mode, after the first solve: the same figures for the inner solver that factors the reduced camera system by the
 * sparse block path (its factor's nonzeros and flops under our ordering, stages, the dimension of its dense top in
 * schur_dim) -- what the roofline of the "reduced_sparse" phase is priced with; all zero when the reduced system is
 * factored densely (then slampp_hip_get_stats has n^3/3).  A handle over several devices answers for member 0 (the
 * reduced system is the same on every member). */
int slampp_hip_get_reduced_stats(const slampp_hip_solver *p_solver, slampp_hip_stats *p_stats);

/* device-side phase timing (the counterpart of the reference's __SCHUR_PROFILING / CTimerSampler
 * phase timers, LinearSolver_Schur.h:1681-1912, Timer.h:391): with option "profile" = 1 every phase
 * of factor_solve is bracketed by HIP events on the solver's stream; the totals are collected at
 * slampp_hip_sync().  Phases: factor_leaves, factor_rest (with "profile" = 2: factor_wide, factor_upper), forward, backward (sparse path);
 * schur_init, schur_tiles (the landmark-major assembly) and / or schur_points, schur_gather, schur_rhs (contribution lists),
 * reduced_sparse or dense_chol + dense_solve, backsubst (Schur path); a phase that launches nothing is left out.
 * An event pair costs microseconds of stream time: "profile" = 3 keeps only the phase of the kernel that moves most of a
 * step's bytes or flops (factor_leaves; schur_tiles / schur_gather; dense_chol) -- what a timed region should carry. */
typedef struct slampp_hip_phase_time {
	char name[32];
	int64_t n_count;      /* times the phase ran */
	double f_total_ms;    /* summed device time */
} slampp_hip_phase_time;
int slampp_hip_get_profile(slampp_hip_solver *p_solver, slampp_hip_phase_time *p_phases, int n_max_phases,
	int *p_phase_num, int b_reset);

/* The same totals under the names the reference prints with __SCHUR_PROFILING (LinearSolver_Schur.h:1681-1912, in its order):
 *   "reperm", "slice", "transpose"   always 0: the packed block-CSC with the cameras first is [A U; C] already
 *   "inverse + multiply + add"       C^-1, U C^-1, (U C^-1) U^T and A - ... are one pass here (schur_init + schur_tiles /
 *                                    schur_points + schur_gather); the reference's lines "inverse", "diag gemm", "scale",
 *                                    "gemm" and "add" added up are its counterpart
 *   "RHS prep"                       schur_rhs (zero where the landmark-major assembly forms the right-hand side on its way)
 *   "cholsol"                        reduced_sparse, or dense_chol + dense_solve
 *   "dy solve"                       backsubst
 * and, in sparse mode, CHOLMOD's two numeric phases (LinearSolver_CholMod.cpp:322-347): "factorize" (with the forward
 * substitution, which is fused into it) and "solve" (the backward one).  Nothing is reset by this call. */
int slampp_hip_get_profile_reference_names(slampp_hip_solver *p_solver, slampp_hip_phase_time *p_phases, int n_max_phases,
	int *p_phase_num);

/* Lambda and eta assembled on the device from per-edge Jacobians (first row after the
 * solve): replaces the host loop that computes every edge's Hessian blocks and the reduction that sums
 * them into Lambda (include/slam/BaseTypes_Binary.h:759-840 Calculate_Hessians_v2,
 * include/slam/NonlinearSolver_Lambda_Base.h:1634-1688 Refresh_Lambda, :1520-1580 the unary factor) for one
 * homogeneous set of binary edges, so that Lambda never visits the host between linearization and solve.
 *
 * create: after slampp_hip_set_structure().  Edge e joins block columns p_vertex0[e] and p_vertex1[e] of
 * Lambda (all vertex0 of one dimension d0, all vertex1 of one dimension d1, both <= 7) with an
 * n_residual_dim-vector residual (<= 8); Lambda must hold the block (min, max) of every edge.
 *
 * assemble: device arrays, edge-major, every matrix column-major as the reference's Eigen types are:
 *   p_J0_dev [n_edges][rd x d0], p_J1_dev [n_edges][rd x d1], p_sigma_inv_dev [n_edges][rd x rd],
 *   p_error_dev [n_edges][rd], p_weight_dev [n_edges] robust weights or NULL (= 1).
 * p_unary_factor (host, d x d column-major, or NULL) and p_unary_error (host, d, or NULL) anchor
 * block column n_unary_vertex: U^T U is added to its diagonal block and the error to its eta.
 * Writes the packed block values of Lambda (the layout slampp_hip_factor_solve_device reads) and eta;
 * with b_accumulate != 0 adds to what the two arrays hold instead (a second edge set of the same Lambda).
 * Sums run in a fixed order: results are bit-reproducible.  Enqueue-only, on the solver's stream.
 *
 * Alignment of p_J0_dev, p_J1_dev, p_sigma_inv_dev and p_error_dev: where the handle formed vertex groups
 * (slampp_hip_assembly_get_info: n_groups > 0) and n_residual_dim is 2 or 6, the group kernel copies the four arrays
 * with 16-byte loads, and each must start at a multiple of 16 bytes -- what hipMalloc and every allocator on top of it
 * give; a pointer into the middle of a larger allocation need not.  slampp_hip_assemble_device_async and
 * slampp_hip_assemble_sets_device_async return SLAMPP_HIP_ERR_INVALID otherwise, before anything is enqueued.  In every
 * other case the natural alignment of a double is enough. */
/* Levenberg-Marquardt damping of device-resident values (the ones slampp_hip_assemble_device_async wrote): adds
 * f_alpha to the diagonal of the diagonal blocks of block columns [n_first_vertex, n_last_vertex) -- the reference's
 * ApplyDamping(r_lambda, f_alpha, n_first_vertex, n_last_vertex), include/slam/NonlinearSolver_Lambda_LM.h:228-239,
 * which it runs on the host matrix between Refresh_Lambda and the linear solve.  A negative f_alpha takes it back
 * out (the LM loop re-damps the same Lambda).  Enqueue-only, on the solver's stream; needs set_structure only. */
int slampp_hip_apply_damping_device_async(slampp_hip_solver *p_solver, double *p_values_dev, double f_alpha,
	int64_t n_first_vertex, int64_t n_last_vertex);

typedef struct slampp_hip_assembly slampp_hip_assembly; /* opaque */
int slampp_hip_assembly_create(slampp_hip_solver *p_solver, slampp_hip_assembly **pp_assembly, int64_t n_edges,
	const int64_t *p_vertex0, const int64_t *p_vertex1, int n_residual_dim);
void slampp_hip_assembly_destroy(slampp_hip_assembly *p_assembly); /* in either order with its solver's destroy */
/* What create built, by the kernel that takes it (read-only): consecutive vertices with few edges go
 * to the group kernel (n_groups groups of at most n_grp_cap_edges edges, one package of n_grp_pkg_stride words each; no
 * groups where n_grp_cap_edges < 8 or option "assembly_groups" is 0); of the others, n_long vertices of dimension
 * n_long_dim with 96 edges or more to the edge-parallel kernel, n_small to the packed kernel (n_small_elems lanes each),
 * n_plain_diag to the one-wave kernel; the n_offdiag off-diagonal blocks outside the groups (n_off_elems: the largest, in
 * elements) to the packed kernel (b_offdiag_packed) or the one-wave kernel. */
typedef struct slampp_hip_assembly_info {
	int rd, d0, d1; /* n_residual_dim and the two vertex dimensions of the set */
	int n_grp_cap_edges, n_grp_pkg_stride;
	int n_long_dim, n_small_elems, n_off_elems, b_offdiag_packed;
	int n_pad;
	int64_t n_groups, n_long, n_small, n_plain_diag, n_offdiag;
} slampp_hip_assembly_info;
int slampp_hip_assembly_get_info(const slampp_hip_assembly *p_assembly, slampp_hip_assembly_info *p_info);
int slampp_hip_assemble_device_async(slampp_hip_assembly *p_assembly, const double *p_J0_dev, const double *p_J1_dev,
	const double *p_sigma_inv_dev, const double *p_error_dev, const double *p_weight_dev, int64_t n_unary_vertex,
	const double *p_unary_factor, const double *p_unary_error, double *p_values_dev, double *p_eta_dev, int b_accumulate);

/* Every edge type of a graph in one call, as the reference's Refresh_Lambda reduces them all
 * (include/slam/NonlinearSolver_Lambda_Base.h:1659-1688: one loop per edge pool of the typelist): n_sets homogeneous
 * edge sets of the same Lambda -- pose-pose and pose-landmark edges, say -- each with its own assembly handle and
 * device arrays as above.  Lambda and eta start from zero (b_accumulate != 0: from what the arrays hold), every set is
 * added in the order given (fixed order: bit-reproducible), the unary factor with the first.  Enqueue-only. */
typedef struct slampp_hip_edge_set {
	slampp_hip_assembly *p_assembly;
	const double *p_J0_dev, *p_J1_dev, *p_sigma_inv_dev, *p_error_dev, *p_weight_dev; /* as slampp_hip_assemble_device_async */
} slampp_hip_edge_set;
int slampp_hip_assemble_sets_device_async(const slampp_hip_edge_set *p_sets, int n_sets, int64_t n_unary_vertex,
	const double *p_unary_factor, const double *p_unary_error, double *p_values_dev, double *p_eta_dev, int b_accumulate);

/* The two ends of a Gauss-Newton / LM iteration, so that the loop
 *   linearize -> assemble -> (damp) -> factor_solve -> state_plus -> chi_squared
 * runs without the states, the Jacobians, Lambda or dx leaving the device.
 *
 * linearize: every edge's error and Jacobians from the vertex states -- Calculate_Jacobians_Expectation_Error of the
 * reference's three workhorse edges -- for the edge set of an assembly handle, which knows the edges' vertices and dimensions:
 *   SLAMPP_HIP_EDGE_SE2      CEdgePose2D (SE2_Types.h:308-318, 2DSolverBase.h:372-424): h = (R^T(th0) (p1 - p0),
 *                            f_ClampAngle_2Pi(th1 - th0)), err = z - h, its angle through f_ClampAngularError_2Pi
 *                            (2DSolverBase.h:44-94); the Jacobians are the closed forms of lines 412-423, derivatives with
 *                            respect to an additive perturbation of the state;
 *   SLAMPP_HIP_EDGE_SE3      CEdgePose3D (SE3_Types.h:265-287, 3DSolverBase.h:806-946): h = (R0^T (t1 - t0), Log(R0^T R1)), Log
 *                            the principal logarithm (the quaternion with w >= 0: f_AxisAngle_to_Quat, 3DSolverBase.h:476-519),
 *                            err = (z_t - h_t, Log(Exp(z_r) Exp(h_r)^T)); J0 = dh(x0 (+) e, x1) / de and J1 = dh(x0, x1 (+) e) / de
 *                            at e = 0, (+) being Relative_to_Absolute: t <- t + R e_t, R <- R Exp(e_r);
 *   SLAMPP_HIP_EDGE_P2C_XYZ  CEdgeP2C3D (BA_Types.h:403-505, BASolverBase.h:259-327, 558-619; DATA_UPSIDE_DOWN off): x = R X + t,
 *                            pinhole projection with the camera's intrinsics (fx, fy, cx, cy, k), then the one-coefficient
 *                            radial term with k / ((fx + fy) / 2); err = z - projection; the camera moves by the SE(3) (+)
 *                            above, the point additively;
 *   SLAMPP_HIP_EDGE_POSE_LANDMARK_2D  CEdgePoseLandmark2D (SE2_Types.h:340-596, 2DSolverBase.h:443-496), range and bearing:
 *                            (de, dn) = l - p, r = sqrt(de^2 + dn^2), h = (r, f_ClampAngle_2Pi(atan2(dn, de) - theta)); an
 *                            |r| < 1e-5 is replaced by 1e-5, in h and in the denominators of both Jacobians (:475-495);
 *                            err = z - h, its angle through f_ClampAngularError_2Pi; the Jacobians are the closed forms of
 *                            lines 488-494, for additive perturbations of pose and landmark;
 *   SLAMPP_HIP_EDGE_POSE_LANDMARK_3D  CEdgePoseLandmark3D (SE3_Types.h:444-603, 3DSolverBase.h:1528-1638): h = R0^T (X - t0),
 *                            err = z - h; J0 = [-I, [h]x] under the SE(3) (+) above, J1 = R0^T;
 *   SLAMPP_HIP_EDGE_P2SC_XYZ CEdgeP2SC3D (BA_Types.h:705-850, BASolverBase.h:462-537, 781-841), the stereo camera: the left
 *                            image is p = (fx x / z, fy y / z), projection = c + (1 + k' |p|) p with k' = k / ((fx + fy) / 2) --
 *                            the radial term is linear in |p| here (:516-517), where P2C_XYZ has |p|^2 (:309-312); the right
 *                            image is the same projection of the camera-frame point moved by -baseline along the camera's x
 *                            axis (the reference takes b R.row(0) off the world point, :522, which is the same); h = (u, v) of
 *                            the left image and u of the right one, err = z - h; the camera moves by the SE(3) (+), the point
 *                            additively.
 * Where the reference differences forwards with a step of 1e-9 (SE3, P2C_XYZ, POSE_LANDMARK_3D, P2SC_XYZ: 3DSolverBase.h:1331-1371,
 * 1602-1637, BASolverBase.h:577-619, 801-840; good to about 1e-7), these are the exact derivatives of the same functions in
 * closed form.
 *   p_state_dev        n_scalars doubles in Lambda's scalar order -- the layout of eta and dx: the state of block column v at
 *                      its scalar offset (for these vertex types the state dimension is the block dimension);
 *   p_measurement_dev  [n_edges][3 | 6 (xyz, axis-angle) | 2 | 2 (range, bearing) | 3 (xyz) | 3 (u, v, u right)];
 *   p_params_dev       NULL but for P2C_XYZ and P2SC_XYZ: the five intrinsics (fx, fy, cx, cy, k) of the camera at block column c
 *                      at p_params_dev + 5 c, for P2SC_XYZ the six (fx, fy, cx, cy, k, baseline) at p_params_dev + 6 c (only
 *                      the entries of block columns that are some edge's vertex 0 are read);
 *   p_J0_dev [n_edges][rd x d0], p_J1_dev [n_edges][rd x d1], p_error_dev [n_edges][rd]: written, in the layout
 *                      slampp_hip_assemble_device_async reads (edge-major, matrices column-major).
 * A lane computes an edge; a workgroup stages the outputs of its 64 edges in LDS and writes whole lines.  No atomics: the same
 * call twice gives the same bits, and an edge's results do not depend on the other edges of the set.
 * SLAMPP_HIP_ERR_INVALID (text under "linearize"): a null handle or a null required pointer, an assembly that a set_structure
 * has outdated, an unknown type, a type whose (d0, d1, rd) are not the handle's, P2C_XYZ or P2SC_XYZ without p_params_dev.
 * Enqueue-only on the solver's stream.
 * The value 4 is no edge type and stays unassigned: callers and tests use it as the unknown type ("linearize: unknown edge
 * type", checked before the dimensions), so the types added later begin at 5. */
#define SLAMPP_HIP_EDGE_SE2      1  /* CEdgePose2D: d0 = d1 = 3, rd = 3, measurement 3 doubles          */
#define SLAMPP_HIP_EDGE_SE3      2  /* CEdgePose3D: d0 = d1 = 6, rd = 6, measurement 6 (xyz, axis-angle) */
#define SLAMPP_HIP_EDGE_P2C_XYZ  3  /* CEdgeP2C3D:  d0 = 6 (camera), d1 = 3 (point), rd = 2, measurement 2 */
#define SLAMPP_HIP_EDGE_POSE_LANDMARK_2D 5  /* CEdgePoseLandmark2D: d0 = 3 (pose), d1 = 2 (landmark), rd = 2, measurement 2 */
#define SLAMPP_HIP_EDGE_POSE_LANDMARK_3D 6  /* CEdgePoseLandmark3D: d0 = 6 (pose), d1 = 3 (landmark), rd = 3, measurement 3 */
#define SLAMPP_HIP_EDGE_P2SC_XYZ 7  /* CEdgeP2SC3D: d0 = 6 (camera), d1 = 3 (point), rd = 3, measurement 3, six parameters */
int slampp_hip_linearize_device_async(slampp_hip_assembly *p_assembly, int n_edge_type, const double *p_state_dev,
	const double *p_measurement_dev, const double *p_params_dev, double *p_J0_dev, double *p_J1_dev, double *p_error_dev);

/* out = state (+) f_scale dx on block columns [n_first_vertex, n_last_vertex) -- the range convention of
 * slampp_hip_apply_damping_device_async -- on the manifold of the vertex type: Operator_Plus of the reference's vertices, which
 * PushValuesInGraphSystem runs over the vertex pool (NonlinearSolver_Base.h); f_scale = -1 is Operator_Minus, the LM roll-back.
 * State and dx in the layout of eta.  p_state_out_dev may be p_state_dev (in place, to the bits of out of place); otherwise the
 * two must not overlap, and dx overlaps neither.  Block columns outside the range are not written (a graph with cameras and
 * points takes two calls).  Needs slampp_hip_set_structure only.  A lane per block column; no atomics.
 * SLAMPP_HIP_ERR_INVALID (text under "state_plus"): a null pointer, no structure, an unknown type, a range outside
 * [0, n_bcols] or with first > last, a block column in the range whose dimension is not the type's (3 for SE2, 6 for SE3, above 8
 * for EUCLIDEAN), arrays that overlap in part.  Enqueue-only on the solver's stream, but for the first call after a
 * set_structure, which uploads the block columns' offsets and waits for that copy. */
#define SLAMPP_HIP_VERTEX_EUCLIDEAN 0  /* x += s dx (CVertexXYZ; any block dimension up to 8)                      */
#define SLAMPP_HIP_VERTEX_SE2       1  /* x += s dx, theta = f_ClampAngle_2Pi(theta)   (SE2_Types.h:70-74)          */
#define SLAMPP_HIP_VERTEX_SE3       2  /* Relative_to_Absolute(x, s dx) (CVertexPose3D, CVertexCam: SE3_Types.h:45-48) */
int slampp_hip_state_plus_device_async(slampp_hip_solver *p_solver, int n_vertex_type, int64_t n_first_vertex,
	int64_t n_last_vertex, const double *p_state_dev, const double *p_dx_dev, double f_scale, double *p_state_out_dev);

/* *p_out_dev = sum over the edges of the handle of w_e err_e^T Sigma_e^-1 err_e (p_weight_dev NULL: w = 1) -- f_Chi_Squared_Error
 * of the edges summed over the edge pool (NonlinearSolver_Lambda.h f_Chi_Squared_Error_Denorm), on the error array
 * slampp_hip_linearize_device_async wrote and the Sigma^-1 array the assembly reads.  Two passes as in
 * slampp_hip_dot_device_async: a lane adds the terms of its edges, then the sums are added in a fixed order that depends on
 * n_edges alone -- bit-reproducible, no atomics.  Any edge set (rd <= 8).  SLAMPP_HIP_ERR_INVALID (text under "chi2"): a null
 * handle or pointer, an outdated assembly.  Enqueue-only on the solver's stream. */
int slampp_hip_chi_squared_device_async(slampp_hip_assembly *p_assembly, const double *p_sigma_inv_dev,
	const double *p_error_dev, const double *p_weight_dev /* or NULL */, double *p_out_dev);

/* The Levenberg-Marquardt loop decided on the device: accept or reject,
 * the next alpha and nu, convergence and the budget of extra iterations are decided by kernels on a caller-owned block of
 * SLAMPP_HIP_LM_SCALARS doubles in device memory, so that a caller enqueues N iterations and waits once.  The rule is the
 * reference's CLevenbergMarquardt_Baseline (include/slam/NonlinearSolver_Lambda_LM.h:151-223) inside the loop of
 * CNonlinearSolver_Lambda_LM::Optimize (:915-1115).  Counters and flags are stored as doubles holding integers. */
#define SLAMPP_HIP_LM_ALPHA        0  /* the damping the next solve uses                                              */
#define SLAMPP_HIP_LM_NU           1  /* the factor of the next rejected step (m_nu)                                  */
#define SLAMPP_HIP_LM_LAST_ERROR   2  /* chi^2 at the state (f_last_error)                                            */
#define SLAMPP_HIP_LM_ERROR        3  /* chi^2 at the trial state of the last decision                                */
#define SLAMPP_HIP_LM_DX_DX        4  /* dx^T dx of the last solve                                                    */
#define SLAMPP_HIP_LM_DX_ETA       5  /* dx^T eta of the last solve                                                   */
#define SLAMPP_HIP_LM_RHO          6  /* the gain ratio of the last decision (0 where none was formed)                */
#define SLAMPP_HIP_LM_ACCEPTED     7  /* 1: the last decision accepted its step (slampp_hip_lm_commit_device_async copies) */
#define SLAMPP_HIP_LM_STATUS       8  /* SLAMPP_HIP_LM_STATUS_*                                                       */
#define SLAMPP_HIP_LM_N_ROUNDS     9  /* decisions entered with status 0                                              */
#define SLAMPP_HIP_LM_N_ACCEPTED   10
#define SLAMPP_HIP_LM_N_REJECTED   11
#define SLAMPP_HIP_LM_ROUNDS_LEFT  12 /* iterations left (n_max_iteration_num - n_iteration)                          */
#define SLAMPP_HIP_LM_EXTRA_LEFT   13 /* extra iterations still to be granted on rejected steps (fail)                */
#define SLAMPP_HIP_LM_MIN_DX_NORM  14 /* f_min_dx_norm                                                                */
#define SLAMPP_HIP_LM_N_RECORDS    15 /* trace records appended (those beyond the capacity were counted and dropped)  */
#define SLAMPP_HIP_LM_SCALARS      16
#define SLAMPP_HIP_LM_STATUS_RUNNING     0
#define SLAMPP_HIP_LM_STATUS_CONVERGED   1  /* |dx| <= f_min_dx_norm: the step was not applied (:1054)                */
#define SLAMPP_HIP_LM_STATUS_NOT_POSDEF  2  /* the factorization failed (:972)                                        */
#define SLAMPP_HIP_LM_STATUS_BUDGET      3  /* n_max_iteration_num iterations, and the extra ones granted, are used up */
/* a trace record: SLAMPP_HIP_LM_TRACE_RECORD doubles per decision entered with status 0 */
#define SLAMPP_HIP_LM_TRACE_ALPHA       0  /* the alpha the solve used   */
#define SLAMPP_HIP_LM_TRACE_ERROR       1  /* chi^2 at the trial state   */
#define SLAMPP_HIP_LM_TRACE_RHO         2
#define SLAMPP_HIP_LM_TRACE_DX_NORM     3  /* sqrt(dx^T dx)              */
#define SLAMPP_HIP_LM_TRACE_ACCEPTED    4
#define SLAMPP_HIP_LM_TRACE_STATUS      5  /* the status after           */
#define SLAMPP_HIP_LM_TRACE_LAST_ERROR  6  /* LAST_ERROR after           */
#define SLAMPP_HIP_LM_TRACE_NU          7  /* nu after                   */
#define SLAMPP_HIP_LM_TRACE_RECORD      8
#define SLAMPP_HIP_LM_MAX_SETS          8

/* The building blocks; each is enqueue-only on the solver's stream, refuses on the host before anything is enqueued
 * (SLAMPP_HIP_ERR_INVALID, text under "lm"), uses no atomics, and gives the same bits when called twice.
 *
 * edge_errors: the error array of slampp_hip_linearize_device_async, to its bits, without the Jacobians -- all that the
 * reference's f_Chi_Squared_Error evaluates at a trial state.  The same kernels with the Jacobian stores compiled out.
 *
 * apply_damping_scalar: slampp_hip_apply_damping_device_async with the damping f_scale * *p_alpha_dev, *p_alpha_dev read
 * on the device when the kernel runs (f_scale = -1 takes the same damping back out).
 *
 * lm_initial_damping: *p_alpha_out_dev = f_tau * max over the edges of all n_sets (<= SLAMPP_HIP_LM_MAX_SETS) sets of the
 * largest diagonal entry of w_e J0^T Omega J0 and of w_e J1^T Omega J1 -- f_InitialDamping (:151-199) through
 * f_Max_VertexHessianDiagValue (BaseTypes_Binary.h:1200-1222): the maximum starts from 0, a NaN does not enter it, the unary
 * factor is no edge and does not count.  Any sets with rd, d0, d1 <= 8; the Jacobians are those the sets' arrays hold.
 *
 * lm_gain: p_lm_dev[DX_DX] = dx^T dx and p_lm_dev[DX_ETA] = dx^T eta over the solver's n_scalars entries in one pass, with
 * the partition and the summation trees of slampp_hip_dot_device_async (they depend on n alone).  Writes nothing when
 * p_lm_dev[STATUS] is not 0.
 *
 * lm_decide: one decision by one lane.  With STATUS != 0 it clears ACCEPTED and returns.  Otherwise ERROR = the n_parts
 * chi^2 parts added in index order, N_ROUNDS counts up, and in this order:
 *   the handle's not-positive-definite flag is set (the one slampp_hip_sync reports; in Schur mode the outer solver's)
 *                                        -> STATUS = 2, ACCEPTED = 0, RHO = 0;
 *   sqrt(DX_DX) <= MIN_DX_NORM           -> STATUS = 1, ACCEPTED = 0, RHO = 0  (the step is not applied);
 *   rho = (LAST_ERROR - ERROR) / (ALPHA * DX_DX + DX_ETA); if(rho > 0), the only test -- a NaN rejects:
 *     accepted:  t = 2 rho - 1, ALPHA *= max(1 / 3., 1 - t * t * t), NU = 2, LAST_ERROR = ERROR, N_ACCEPTED counts up
 *                (the cube is two multiplications where the reference calls pow(t, 3): at most an ulp apart);
 *     rejected:  ALPHA *= NU, NU *= 2, N_REJECTED counts up, and while EXTRA_LEFT > 0 one unit moves from it to ROUNDS_LEFT;
 *   ROUNDS_LEFT counts down; at 0, STATUS = 3.
 * Every decision entered with STATUS = 0 writes one record (SLAMPP_HIP_LM_TRACE_*) at index N_RECORDS of p_trace_dev where
 * p_trace_dev is not NULL and N_RECORDS < n_trace_capacity, and counts N_RECORDS up either way.  Needs an analyzed handle.
 *
 * lm_commit: state = trial (n_scalars doubles) where ACCEPTED != 0; otherwise nothing is written, so that a rejected step
 * leaves the state's bits alone -- the reference's Save_State / Load_State (:1062, 1100) without the round trip through
 * x (+) dx (-) dx, which is not x to the bit on SE(3).  16 bytes per lane where the two arrays share their alignment. */
int slampp_hip_edge_errors_device_async(slampp_hip_assembly *p_assembly, int n_edge_type, const double *p_state_dev,
	const double *p_measurement_dev, const double *p_params_dev, double *p_error_dev);
int slampp_hip_apply_damping_scalar_device_async(slampp_hip_solver *p_solver, double *p_values_dev, const double *p_alpha_dev,
	double f_scale, int64_t n_first_vertex, int64_t n_last_vertex);
int slampp_hip_lm_initial_damping_device_async(const slampp_hip_edge_set *p_sets, int n_sets, double f_tau, double *p_alpha_out_dev);
int slampp_hip_lm_gain_device_async(slampp_hip_solver *p_solver, const double *p_dx_dev, const double *p_eta_dev, double *p_lm_dev);
int slampp_hip_lm_decide_device_async(slampp_hip_solver *p_solver, double *p_lm_dev, const double *p_chi_parts_dev, int n_parts,
	double *p_trace_dev /* or NULL */, int64_t n_trace_capacity);
int slampp_hip_lm_commit_device_async(slampp_hip_solver *p_solver, const double *p_lm_dev, double *p_state_dev,
	const double *p_trial_dev);

/* The loop.  A problem names everything an iteration touches; the arrays are the caller's, in device memory but for the
 * unary factor and error (host, as in slampp_hip_assemble_device_async) and the lists of sets and ranges (host). */
typedef struct slampp_hip_lm_edge_set {
	slampp_hip_assembly *p_assembly;
	int n_edge_type;                               /* SLAMPP_HIP_EDGE_*, fitting the assembly's dimensions */
	const double *p_measurement_dev, *p_params_dev /* P2C_XYZ only */, *p_sigma_inv_dev, *p_weight_dev /* or NULL */;
	double *p_J0_dev, *p_J1_dev, *p_error_dev;     /* scratch: written by every iteration */
} slampp_hip_lm_edge_set;
typedef struct slampp_hip_lm_vertex_range {
	int n_vertex_type;                             /* SLAMPP_HIP_VERTEX_* */
	int64_t n_first_vertex, n_last_vertex;
} slampp_hip_lm_vertex_range;
typedef struct slampp_hip_lm_problem {
	slampp_hip_solver *p_solver;
	int n_sets;                                    /* 1 to SLAMPP_HIP_LM_MAX_SETS */
	const slampp_hip_lm_edge_set *p_sets;
	int n_ranges;                                  /* together the ranges cover [0, n_bcols) exactly once */
	const slampp_hip_lm_vertex_range *p_ranges;
	int64_t n_unary_vertex;                        /* -1: none */
	const double *p_unary_factor, *p_unary_error;  /* host, or NULL */
	double *p_state_dev, *p_trial_dev;             /* n_scalars each; trial is scratch */
	double *p_values_dev, *p_eta_dev, *p_dx_dev;   /* scratch: Lambda's packed values, eta and the step */
	double *p_lm_dev;                              /* SLAMPP_HIP_LM_SCALARS */
	double *p_chi_parts_dev;                       /* n_sets */
	double *p_trace_dev;                           /* n_trace_capacity records, or NULL */
	int64_t n_trace_capacity;
} slampp_hip_lm_problem;
/* begin: the scalars of a new loop.  ALPHA = f_tau * the initial damping of a linearization of the start state where
 * f_tau > 0 (the reference: 1e-3), otherwise f_alpha; NU = 2; LAST_ERROR = chi^2 of the start state; MIN_DX_NORM, ROUNDS_LEFT =
 * n_max_iterations (STATUS = 3 at once where that is not positive) and EXTRA_LEFT = n_extra_on_reject (the reference: 10);
 * everything else 0.  The trace starts over.
 *
 * iterate: n_rounds times  linearize the state -> assemble -> dx = eta -> damping from ALPHA -> factor_solve -> gain ->
 * state_plus into trial over every range -> errors at trial -> chi^2 per set -> decide -> commit.  The sequence is fixed:
 * after a rejected step the unchanged state is linearized again where the reference keeps its Jacobians (DESIGN.md section
 * 4.10 has the cost).  Once STATUS is not 0 the remaining rounds change nothing the caller can see: state, scalars and trace
 * keep their bits, the scratch arrays are rewritten with the same system's values.  The caller waits with slampp_hip_sync,
 * which reports SLAMPP_HIP_NOT_POSDEF as after any factorization.  CNonlinearSolver_Lambda_LM::Optimize(n_max, f_min_dx_norm)
 * is begin(0, 1e-3, f_min_dx_norm, n_max, 10) and iterate(n_max + 10).
 *
 * SLAMPP_HIP_ERR_INVALID (text under "lm"): a null handle or required pointer, an outdated assembly or one of another
 * solver, no set or more than SLAMPP_HIP_LM_MAX_SETS, an edge type that does not fit its assembly, vertex ranges that do not
 * cover [0, n_bcols) exactly once or whose types do not fit the block dimensions, state, trial and dx overlapping, a handle
 * that was not analyzed, n_rounds <= 0, an edge set whose assembly has a robust kernel (slampp_hip_assembly_set_robust, below:
 * the loop then computes the set's weights itself) and a weight array as well.  SLAMPP_HIP_ERR_UNSUPPORTED: a handle over several devices, or one with an all-reduce
 * callback (landmark shards).  Both sparse and Schur mode are served. */
int slampp_hip_lm_begin_device_async(const slampp_hip_lm_problem *p_problem, double f_alpha, double f_tau, double f_min_dx_norm,
	int n_max_iterations, int n_extra_on_reject);
int slampp_hip_lm_iterate_device_async(const slampp_hip_lm_problem *p_problem, int n_rounds);

/* Robust kernels on the device: the per-edge weight that the assembly, chi^2
 * and the initial damping already take, computed where the errors are, so that the loop above stays on the device once an edge is
 * an outlier.  The reference's CEdgePose3D is such an edge (SE3_Types.h:128-129: CBaseEdge::Robust with
 * CRobustify_ErrorNorm_Default<CCTFraction<30, 100>, CHuberLossd>): every Calculate_Hessians_v2 multiplies its blocks by
 * w = Huber(|err| / 0.3) (BaseTypes_Binary.h:759-848).
 *
 * A specification is set on an assembly handle; with one set the handle owns a device array of n_edges weights (freed by
 * set_robust(NULL) and with the handle).  w(s), the expressions of the reference's operator () in include/geometry/RobustLoss.h,
 * evaluated in their order without contraction, a = f_param:
 *   SLAMPP_HIP_ROBUST_HUBER   s <= a ? 1 : a / s                     CHuberLoss, :103          (default a = 1.345)
 *   SLAMPP_HIP_ROBUST_CAUCHY  a a / (a a + s s)                      CCauchyLoss, :153         (2.385)
 *   SLAMPP_HIP_ROBUST_TUKEY   s <= a ? (1 - s s / (a a))^2 : 0       CTukeyBiweightLoss, :206  (4.685)
 *   SLAMPP_HIP_ROBUST_WELSCH  exp(-s s / (a a))                      CWelschLoss, :433         (2.985)
 * What s is:
 *   SLAMPP_HIP_ROBUST_BASIS_ERROR_NORM   |err|_2 / f_scale            CRobustify_ErrorNorm_Default, slam/RobustUtils.h:397-399
 *                                        (Sigma^-1 is not read)
 *   SLAMPP_HIP_ROBUST_BASIS_CHI2         err^T Sigma^-1 err / f_scale CRobustify_Chi2_Default, :531-534 -- the squared form
 *                                        handed to the kernel as it stands
 *   SLAMPP_HIP_ROBUST_BASIS_MAHALANOBIS  sqrt(err^T Sigma^-1 err) / f_scale   no counterpart in the reference: the usual
 *                                        convention, and the only basis for which w(s) Sigma^-1 err is the gradient of a cost
 * How the loop of slampp_hip_lm_* uses the weight:
 *   SLAMPP_HIP_ROBUST_MODE_REFERENCE  line for line with the reference: w is the assembly's weight array, so Lambda gets w and
 *                                     vertex 0's eta gets w^2 (the reference's own doubling, BaseTypes_Binary.h:813-815); the
 *                                     initial damping reads the weighted blocks (:1200-1222); chi^2 is not weighted
 *                                     (f_Chi_Squared_Error of the robust edge, SE3_Types.h:323-331).  Any basis.
 *   SLAMPP_HIP_ROBUST_MODE_LOSS       a robust cost is minimised: J0, J1 and err are scaled by sqrt(w) in place (the reference's
 *                                     device for its A-solver, BaseTypes.h:1478-1483) and assembled without weights, so that
 *                                     Lambda = sum w J^T Sigma^-1 J and eta = sum w J^T Sigma^-1 err on both vertices; the loop
 *                                     compares sum 2 f_scale^2 rho(s) of the unscaled error.  MAHALANOBIS only.
 * rho has rho' = s w(s) and rho(0) = 0 (not the reference's v_Loss, whose Welsch is a copy of Fair's):
 *   Huber s s / 2 up to a, a (s - a / 2) beyond; Cauchy (a a / 2) log(1 + s s / (a a)); Tukey (a a / 6) (1 - (1 - s s / (a a))^3)
 *   up to a, a a / 6 beyond; Welsch (a a / 2) (1 - exp(-s s / (a a))).  Below the threshold of Huber 2 f_scale^2 rho(s) is
 *   err^T Sigma^-1 err.
 *
 * set_robust: copies the specification (NULL: none again) and allocates or frees the weight array; waits for the solver's
 * stream before it frees.  robust_weights (the pointer of the handle's array in *pp_weight_dev, NULL where none is set).
 *
 * The three kernels are enqueue-only on the solver's stream, use no atomics and give the same bits when called twice; an edge's
 * weight does not depend on the other edges of the set.  A workgroup stages the records of its 64 edges (contiguous in memory)
 * through LDS as whole lines and a lane forms its edge's s from its row of the tile.
 *   robust_weights      p_weight_out_dev[e] = w(s_e) (NULL: into the handle's array); p_sigma_inv_dev may be NULL with ERROR_NORM;
 *   robust_scale        p_J0_dev, p_J1_dev and p_error_dev, each element times sqrt(w_e) of its edge, in place (p_weight_dev
 *                       NULL: the handle's array);
 *   robust_chi_squared  *p_out_dev = sum over the edges of 2 f_scale^2 rho(s_e), with the partition and the summation trees of
 *                       slampp_hip_chi_squared_device_async (they depend on n_edges alone).  MAHALANOBIS only.
 * SLAMPP_HIP_ERR_INVALID (text under "robust"), before anything is enqueued: a null handle or required pointer, an outdated
 * assembly, an unknown kernel, basis or mode, a scale or parameter that is not positive (a NaN is not), LOSS with another basis
 * than MAHALANOBIS, robust_chi_squared on another basis, a kernel call on a handle without a specification.
 *
 * In slampp_hip_lm_begin_device_async and slampp_hip_lm_iterate_device_async an edge set whose assembly has a specification
 * gets, after its linearize, robust_weights into the handle's array and (LOSS) robust_scale on its scratch arrays; the assembly
 * and the initial damping take the handle's array (REFERENCE) or none (LOSS); its chi^2 part is the unweighted chi^2 (REFERENCE)
 * or robust_chi_squared (LOSS) of the unscaled errors.  Such a set must leave p_weight_dev NULL.  Sets without a specification
 * run as before, and the two kinds mix in one problem.  The handle's array is scratch as J0, J1 and err are: once STATUS has left 0
 * the rounds still enqueued write the weights of the final state into it, the same values every time. */
#define SLAMPP_HIP_ROBUST_HUBER   1
#define SLAMPP_HIP_ROBUST_CAUCHY  2
#define SLAMPP_HIP_ROBUST_TUKEY   3
#define SLAMPP_HIP_ROBUST_WELSCH  4
#define SLAMPP_HIP_ROBUST_BASIS_ERROR_NORM   1
#define SLAMPP_HIP_ROBUST_BASIS_CHI2         2
#define SLAMPP_HIP_ROBUST_BASIS_MAHALANOBIS  3
#define SLAMPP_HIP_ROBUST_MODE_REFERENCE  1
#define SLAMPP_HIP_ROBUST_MODE_LOSS       2
typedef struct slampp_hip_robust {
	int n_kernel;   /* SLAMPP_HIP_ROBUST_HUBER | _CAUCHY | _TUKEY | _WELSCH */
	int n_basis;    /* SLAMPP_HIP_ROBUST_BASIS_ERROR_NORM | _CHI2 | _MAHALANOBIS */
	int n_mode;     /* SLAMPP_HIP_ROBUST_MODE_REFERENCE | _LOSS */
	double f_scale; /* > 0 */
	double f_param; /* > 0: the loss function's a */
} slampp_hip_robust;
int slampp_hip_assembly_set_robust(slampp_hip_assembly *p_assembly, const slampp_hip_robust *p_robust /* NULL: none again */);
int slampp_hip_assembly_robust_weights(slampp_hip_assembly *p_assembly, const double **pp_weight_dev);
int slampp_hip_robust_weights_device_async(slampp_hip_assembly *p_assembly, const double *p_sigma_inv_dev, const double *p_error_dev,
	double *p_weight_out_dev /* NULL: the handle's own array */);
int slampp_hip_robust_scale_device_async(slampp_hip_assembly *p_assembly, const double *p_weight_dev /* NULL: the handle's */,
	double *p_J0_dev, double *p_J1_dev, double *p_error_dev);
int slampp_hip_robust_chi_squared_device_async(slampp_hip_assembly *p_assembly, const double *p_sigma_inv_dev,
	const double *p_error_dev, double *p_out_dev);

/* Multi-GPU BA (new functionality, no reference counterpart -- SURVEY.md section 8e): every rank
 * holds a landmark shard (its own points + all cameras); the partial reduced camera systems
 * [S | rhs] are summed over ranks by this callback (RCCL all-reduce over xGMI) between the Schur
 * accumulation and the dense factorization.  p_dev: device pointer, n_count doubles, in place,
 * on stream p_hip_stream.  Return 0 on success.  NULL callback = single GPU.
 * What travels is not the dense n x n buffer but the 6x6 (7x7, 3x3) blocks of S that are nonzero on at
 * least one rank, plus the right-hand side: on the first step with a new callback the ranks agree on that
 * set through the same callback (one or two extra, synchronous calls: concatenated block lists when
 * "shard_rank" / "shard_world" are set, else an indicator over the lower triangle of the camera-block grid),
 * so every rank must register its callback before the same step. */
typedef int (*slampp_hip_allreduce_fn)(void *p_context, double *p_dev, size_t n_count, void *p_hip_stream);
int slampp_hip_set_allreduce(slampp_hip_solver *p_solver, slampp_hip_allreduce_fn p_fn, void *p_context);

/* test hook: copies the elimination plan (permutation, factor structure, update lists, schedule)
 * into caller-provided buffers so that tests can replay it on the CPU (oracle/plan_exec.c).
 * First call with all pointers NULL to get the sizes. */
typedef struct slampp_hip_plan_view {
	int64_t n_bcols, l_blocks, n_pairs, n_row_entries, n_stages, n_tasks, n_task_cols, l_values;
	int32_t *p_perm;        /* [n_bcols] perm[new] = old */
	int32_t *p_dim;         /* [n_bcols] block dimension in the new order */
	int64_t *p_lptr;        /* [n_bcols+1] */
	int32_t *p_lrow;        /* [l_blocks] block row (new order), first of every column = diagonal */
	int64_t *p_loff;        /* [l_blocks] offset of the block in the factor values */
	int64_t *p_asrc;        /* [l_blocks] offset in the packed Lambda values, -1 = fill-in; */
	int32_t *p_atrans;      /* [l_blocks] 1 = source block must be transposed */
	int64_t *p_pptr;        /* [l_blocks+1] update pairs of every block */
	int32_t *p_pa, *p_pb;   /* [n_pairs] factor block ids: L(i,c) and L(j,c) */
	int64_t *p_rptr;        /* [n_bcols+1] row lists (forward solve) */
	int32_t *p_rblk;        /* [n_row_entries] */
	int32_t *p_stage_ptr;   /* [n_stages+1] -> tasks */
	int64_t *p_task_ptr;    /* [n_tasks+1] -> task columns */
	int32_t *p_task_cols;   /* [n_task_cols] */
	int32_t *p_dense_pos;   /* [n_bcols] scalar offset of the column in the dense top, -1 = eliminated block by block */
	int64_t dense_dim;      /* scalar dimension of the dense top (0 = none) */
} slampp_hip_plan_view;
int slampp_hip_get_plan(const slampp_hip_solver *p_solver, slampp_hip_plan_view *p_view);

/* the same analysis without a solver or a GPU (host code only): lets the CPU-only test suite
 * check ordering, symbolic factorization and schedule.  n_leaf_size / n_subtree_size <= 0 = default. */
typedef struct slampp_hip_plan slampp_hip_plan;
int slampp_hip_plan_create(slampp_hip_plan **pp_plan, int64_t n_bcols, const int64_t *p_bcol_cumsum,
	const int64_t *p_bcol_ptr, const int32_t *p_brow_idx, int n_leaf_size, int n_subtree_size,
	int n_dense_top_nb /* < 0 = default */);
int slampp_hip_plan_get(const slampp_hip_plan *p_plan, slampp_hip_plan_view *p_view, slampp_hip_stats *p_stats);
void slampp_hip_plan_destroy(slampp_hip_plan *p_plan);

#ifdef __cplusplus
}
#endif

#endif /* SLAMPP_HIP_H_INCLUDED */
