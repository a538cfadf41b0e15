"""Host-side mirror of the reference's linear-solver interface over the C ABI of libslampp_hip.so.

The reference binds a linear solver as a duck-typed template parameter
(/root/reference/include/slam/LinearSolverTags.h:38-135); the C++ binding is
include/slam/LinearSolver_HIP.h.  This module is the same surface for Python callers and for the
parity tests: same method names, same argument meaning (``eta`` is overwritten with the solution),
same error behaviour (``False`` = not positive definite, ``MemoryError`` = std::bad_alloc,
``RuntimeError`` = std::runtime_error) as

* ``CLinearSolver_CholMod`` / ``CLinearSolver_UberBlock``  (LinearSolver_CholMod.h:148-214,
  LinearSolver_UberBlock.h:256-426)  ->  :class:`CLinearSolver_HIP`
* ``CLinearSolver_Schur``  (LinearSolver_Schur.h:1423-1935)  ->  :class:`CLinearSolver_Schur_HIP`
* ``CNonlinearSolver_Lambda::Refresh_Lambda`` (NonlinearSolver_Lambda_Base.h:1634-1688) for one edge set
  ->  :class:`CLambdaAssembly_HIP`
* the two ends of its iteration -- the edges' ``Calculate_Jacobians_Expectation_Error`` and ``f_Chi_Squared_Error``, the
  vertices' ``Operator_Plus`` / ``Operator_Minus`` -- on device-resident states  ->  ``CLambdaAssembly_HIP.Linearize_device``,
  ``.Chi2_device`` and ``State_Plus_device`` of the solver classes

There is no CPU fallback: if the shared library is missing, or there is no GPU, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

try:  # (optional: only the structure keys of this mirror use it)
    import xxhash as _xxhash
except ImportError:
    _xxhash = None

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libslampp_hip.so")

OK, NOT_POSDEF = 0, 1
ERR_INVALID, ERR_ALLOC, ERR_DEVICE, ERR_UNSUPPORTED = -1, -2, -3, -4
MODE_SPARSE, MODE_SCHUR = 0, 1
SOLVE_MAX_COLUMNS = 256    # SLAMPP_HIP_SOLVE_MAX_COLUMNS
HALF_FORWARD, HALF_BACKWARD = 0, 1   # SLAMPP_HIP_HALF_FORWARD, SLAMPP_HIP_HALF_BACKWARD
GRAM_MAX_COLUMNS = 48      # SLAMPP_HIP_GRAM_MAX_COLUMNS
GRAM_CHUNK_ROWS = 2048     # SLAMPP_HIP_GRAM_CHUNK_ROWS
# slampp_hip_multiply: block rows with more blocks than MULTIPLY_LONG_ROW are cut into chunks of MULTIPLY_CHUNK
# (SLAMPP_HIP_MULTIPLY_* in include/slampp_hip.h; the development option "multiply_long_row" lowers the threshold)
MULTIPLY_LONG_ROW, MULTIPLY_CHUNK = 256, 256
EDGE_SE2, EDGE_SE3, EDGE_P2C_XYZ = 1, 2, 3             # SLAMPP_HIP_EDGE_*: CEdgePose2D, CEdgePose3D, CEdgeP2C3D
EDGE_POSE_LANDMARK_2D, EDGE_POSE_LANDMARK_3D, EDGE_P2SC_XYZ = 5, 6, 7   # CEdgePoseLandmark2D, CEdgePoseLandmark3D, CEdgeP2SC3D (4: none)
VERTEX_EUCLIDEAN, VERTEX_SE2, VERTEX_SE3 = 0, 1, 2     # SLAMPP_HIP_VERTEX_*: x + dx, x + dx with the angle clamped, SE(3) (+)
LINEARIZE_TILE_EDGES = 64   # edges of a workgroup of slampp_hip_linearize_device_async (their outputs leave through one LDS tile)
# SLAMPP_HIP_LM_*: the scalars of the device-decided Levenberg-Marquardt loop, its status values and its trace record
(LM_ALPHA, LM_NU, LM_LAST_ERROR, LM_ERROR, LM_DX_DX, LM_DX_ETA, LM_RHO, LM_ACCEPTED, LM_STATUS, LM_N_ROUNDS, LM_N_ACCEPTED,
 LM_N_REJECTED, LM_ROUNDS_LEFT, LM_EXTRA_LEFT, LM_MIN_DX_NORM, LM_N_RECORDS, LM_SCALARS) = range(17)
LM_STATUS_RUNNING, LM_STATUS_CONVERGED, LM_STATUS_NOT_POSDEF, LM_STATUS_BUDGET = range(4)
(LM_TRACE_ALPHA, LM_TRACE_ERROR, LM_TRACE_RHO, LM_TRACE_DX_NORM, LM_TRACE_ACCEPTED, LM_TRACE_STATUS, LM_TRACE_LAST_ERROR,
 LM_TRACE_NU, LM_TRACE_RECORD) = range(9)
LM_MAX_SETS = 8
# SLAMPP_HIP_ROBUST_*: the loss functions (the reference's CHuberLoss, CCauchyLoss, CTukeyBiweightLoss, CWelschLoss), what their
# argument is, and how the LM loop applies the weight; ROBUST_DEFAULT_PARAM: the reference's default a of each
ROBUST_HUBER, ROBUST_CAUCHY, ROBUST_TUKEY, ROBUST_WELSCH = 1, 2, 3, 4
ROBUST_BASIS_ERROR_NORM, ROBUST_BASIS_CHI2, ROBUST_BASIS_MAHALANOBIS = 1, 2, 3
ROBUST_MODE_REFERENCE, ROBUST_MODE_LOSS = 1, 2
ROBUST_DEFAULT_PARAM = {ROBUST_HUBER: 1.345, ROBUST_CAUCHY: 2.385, ROBUST_TUKEY: 4.685, ROBUST_WELSCH: 2.985}


def _hash_array(a: np.ndarray) -> int:
    """Hash of an index array's bytes: xxh3 over the buffer where the module is there (6 ms for C5's 10^7 block rows),
    Python's hash of a copy otherwise (50 ms)."""
    a = np.ascontiguousarray(a)
    if _xxhash is not None:
        return _xxhash.xxh3_64_intdigest(a)
    return hash(a.tobytes())


class Times(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "order_ms", "symbolic_ms", "upload_ms", "factor_ms", "solve_ms", "download_ms",
        "schur_ms", "reduce_ms", "cholsol_ms", "backsubst_ms", "total_ms")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Stats(C.Structure):
    _fields_ = [("n_bcols", C.c_int64), ("n_blocks_upper", C.c_int64), ("n_scalars", C.c_int64),
                ("nnz_upper", C.c_int64), ("l_blocks", C.c_int64), ("l_nnz", C.c_int64),
                ("factor_flops", C.c_double), ("solve_flops", C.c_double),
                ("n_stages", C.c_int64), ("n_tasks", C.c_int64), ("etree_height", C.c_int64),
                ("n_update_pairs", C.c_int64), ("n_cams", C.c_int64), ("n_points", C.c_int64),
                ("n_observations", C.c_int64), ("schur_dim", C.c_int64), ("device_bytes", C.c_int64),
                ("n_bottom_stages", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class PlanView(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_bcols", "l_blocks", "n_pairs", "n_row_entries",
                                         "n_stages", "n_tasks", "n_task_cols", "l_values")] + [
        ("p_perm", C.c_void_p), ("p_dim", C.c_void_p), ("p_lptr", C.c_void_p), ("p_lrow", C.c_void_p),
        ("p_loff", C.c_void_p), ("p_asrc", C.c_void_p), ("p_atrans", C.c_void_p), ("p_pptr", C.c_void_p),
        ("p_pa", C.c_void_p), ("p_pb", C.c_void_p), ("p_rptr", C.c_void_p), ("p_rblk", C.c_void_p),
        ("p_stage_ptr", C.c_void_p), ("p_task_ptr", C.c_void_p), ("p_task_cols", C.c_void_p),
        ("p_dense_pos", C.c_void_p), ("dense_dim", C.c_int64)]


class ShardView(C.Structure):
    _fields_ = [(n, C.c_int64) for n in (
        "n_bcols", "n_blocks", "n_camera_values", "n_value_begin", "n_value_end", "n_camera_scalars", "n_scalar_begin",
        "n_scalar_end", "n_point_begin", "n_point_end")] + [
        ("p_bcol_cumsum", C.c_void_p), ("p_bcol_ptr", C.c_void_p), ("p_brow_idx", C.c_void_p)]


class EdgeSetPtrs(C.Structure):
    _fields_ = [("p_assembly", C.c_void_p), ("p_J0_dev", C.c_void_p), ("p_J1_dev", C.c_void_p), ("p_sigma_inv_dev", C.c_void_p),
                ("p_error_dev", C.c_void_p), ("p_weight_dev", C.c_void_p)]


class AssemblyInfo(C.Structure):
    """slampp_hip_assembly_info"""
    _fields_ = [(n, C.c_int) for n in ("rd", "d0", "d1", "n_grp_cap_edges", "n_grp_pkg_stride", "n_long_dim", "n_small_elems",
                                      "n_off_elems", "b_offdiag_packed", "n_pad")] + [
        (n, C.c_int64) for n in ("n_groups", "n_long", "n_small", "n_plain_diag", "n_offdiag")]


class LmEdgeSet(C.Structure):
    """slampp_hip_lm_edge_set"""
    _fields_ = [("p_assembly", C.c_void_p), ("n_edge_type", C.c_int), ("p_measurement_dev", C.c_void_p), ("p_params_dev", C.c_void_p),
                ("p_sigma_inv_dev", C.c_void_p), ("p_weight_dev", C.c_void_p), ("p_J0_dev", C.c_void_p), ("p_J1_dev", C.c_void_p),
                ("p_error_dev", C.c_void_p)]


class LmVertexRange(C.Structure):
    """slampp_hip_lm_vertex_range"""
    _fields_ = [("n_vertex_type", C.c_int), ("n_first_vertex", C.c_int64), ("n_last_vertex", C.c_int64)]


class LmProblem(C.Structure):
    """slampp_hip_lm_problem"""
    _fields_ = [("p_solver", C.c_void_p), ("n_sets", C.c_int), ("p_sets", C.POINTER(LmEdgeSet)), ("n_ranges", C.c_int),
                ("p_ranges", C.POINTER(LmVertexRange)), ("n_unary_vertex", C.c_int64), ("p_unary_factor", C.c_void_p),
                ("p_unary_error", C.c_void_p), ("p_state_dev", C.c_void_p), ("p_trial_dev", C.c_void_p), ("p_values_dev", C.c_void_p),
                ("p_eta_dev", C.c_void_p), ("p_dx_dev", C.c_void_p), ("p_lm_dev", C.c_void_p), ("p_chi_parts_dev", C.c_void_p),
                ("p_trace_dev", C.c_void_p), ("n_trace_capacity", C.c_int64)]


class Robust(C.Structure):
    """slampp_hip_robust"""
    _fields_ = [("n_kernel", C.c_int), ("n_basis", C.c_int), ("n_mode", C.c_int), ("f_scale", C.c_double), ("f_param", C.c_double)]


class PhaseTime(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("n_count", C.c_int64), ("f_total_ms", C.c_double)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)

# every symbol include/slampp_hip.h declares: (restype, argtypes)
_P = C.c_void_p
ABI = {
    "slampp_hip_create": (C.c_int, [C.POINTER(_P), C.c_int]),
    "slampp_hip_create_multi": (C.c_int, [C.POINTER(_P), C.POINTER(C.c_int), C.c_int]),
    "slampp_hip_group_info": (C.c_int, [_P, C.POINTER(C.c_int), _P, C.c_int, C.POINTER(C.c_char_p)]),
    "slampp_hip_group_exchange_count": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "slampp_hip_group_exchange_selftest": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int64, C.c_char_p, C.c_int]),
    "slampp_hip_landmark_shard": (C.c_int, [C.c_int64, _P, _P, _P, C.c_int64, C.c_int, C.c_int, C.POINTER(ShardView)]),
    "slampp_hip_destroy": (None, [_P]),
    "slampp_hip_free_memory": (C.c_int, [_P]),
    "slampp_hip_last_error": (C.c_char_p, [_P]),
    "slampp_hip_set_option": (C.c_int, [_P, C.c_char_p, C.c_int64]),
    "slampp_hip_set_structure": (C.c_int, [_P, C.c_int64, _P, _P, _P]),
    "slampp_hip_analyze": (C.c_int, [_P, C.c_int, C.c_int64]),
    "slampp_hip_factor_solve": (C.c_int, [_P, _P, _P, C.POINTER(Times)]),
    "slampp_hip_factor_solve_device": (C.c_int, [_P, _P, _P, C.POINTER(Times)]),
    "slampp_hip_host_staging": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "slampp_hip_upload_values_async": (C.c_int, [_P, C.c_int64, C.c_int64]),
    "slampp_hip_solve_again": (C.c_int, [_P, _P]),
    "slampp_hip_solve_again_device_async": (C.c_int, [_P, _P]),
    "slampp_hip_solve_columns_device_async": (C.c_int, [_P, _P, C.c_int64, C.c_int]),
    "slampp_hip_solve_columns": (C.c_int, [_P, _P, C.c_int64, C.c_int]),
    "slampp_hip_solve_half_columns_device_async": (C.c_int, [_P, C.c_int, _P, C.c_int64, C.c_int]),
    "slampp_hip_solve_half_columns": (C.c_int, [_P, C.c_int, _P, C.c_int64, C.c_int]),
    "slampp_hip_gram_device_async": (C.c_int, [_P, _P, C.c_int64, C.c_int, _P, C.c_int64, C.c_int, C.c_int64, _P, C.c_int64]),
    "slampp_hip_pattern_outer_sum_device_async": (C.c_int, [_P, C.c_int, _P, C.c_int64, _P, C.c_int64, _P, C.c_double,
                                                            C.c_double]),
    "slampp_hip_multiply_device_async": (C.c_int, [_P, _P, _P, _P, C.c_double, C.c_double]),
    "slampp_hip_multiply": (C.c_int, [_P, _P, _P, _P, C.c_double, C.c_double]),
    "slampp_hip_pattern_outer_device_async": (C.c_int, [_P, _P, _P, _P, C.c_double, C.c_double]),
    "slampp_hip_pattern_outer": (C.c_int, [_P, _P, _P, _P, C.c_double, C.c_double]),
    "slampp_hip_pattern_outer_batch_device_async": (C.c_int, [_P, C.c_int, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64,
                                                              C.c_double, C.c_double]),
    "slampp_hip_dot_device_async": (C.c_int, [_P, _P, _P, C.c_int64, _P]),
    "slampp_hip_refine_device_async": (C.c_int, [_P, _P, _P, _P, C.c_int, _P]),
    "slampp_hip_refine": (C.c_int, [_P, _P, _P, _P, C.c_int, _P]),
    "slampp_hip_logdet_device_async": (C.c_int, [_P, _P, C.c_int, _P]),
    "slampp_hip_logdet": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_double)]),
    "slampp_hip_factorize": (C.c_int, [_P, _P, _P]),
    "slampp_hip_factor_structure": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), _P, _P, _P, _P, _P]),
    "slampp_hip_schur_set_changed_points": (C.c_int, [_P, _P, C.c_int64]),
    "slampp_hip_solve_marginal_poses": (C.c_int, [_P, _P, _P]),
    "slampp_hip_solve_marginal_poses_device_async": (C.c_int, [_P, _P, _P]),
    "slampp_hip_apply_damping_device_async": (C.c_int, [_P, _P, C.c_double, C.c_int64, C.c_int64]),
    "slampp_hip_marginals": (C.c_int, [_P, _P, _P]),
    "slampp_hip_marginals_device_async": (C.c_int, [_P, _P, _P]),
    "slampp_hip_marginals_pattern": (C.c_int, [_P, _P, _P]),
    "slampp_hip_marginals_pattern_device_async": (C.c_int, [_P, _P, _P]),
    "slampp_hip_marginal_columns": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "slampp_hip_marginal_columns_device_async": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "slampp_hip_marginal_blocks": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P]),
    "slampp_hip_marginal_blocks_device_async": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P]),
    "slampp_hip_schur_marginals": (C.c_int, [_P, _P, _P, _P]),
    "slampp_hip_schur_marginals_device_async": (C.c_int, [_P, _P, _P, _P]),
    "slampp_hip_schur_marginals_pattern": (C.c_int, [_P, _P, _P]),
    "slampp_hip_schur_marginals_pattern_device_async": (C.c_int, [_P, _P, _P]),
    "slampp_hip_schur_marginal_columns": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "slampp_hip_schur_marginal_columns_device_async": (C.c_int, [_P, _P, C.c_int, _P, _P]),
    "slampp_hip_schur_marginal_blocks": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P]),
    "slampp_hip_schur_marginal_blocks_device_async": (C.c_int, [_P, _P, C.c_int64, _P, _P, _P]),
    "slampp_hip_factor_solve_device_async": (C.c_int, [_P, _P, _P]),
    "slampp_hip_sync": (C.c_int, [_P]),
    "slampp_hip_factor_solve_batch_device_async": (C.c_int, [_P, C.c_int, _P, C.c_int64, _P, C.c_int64]),
    "slampp_hip_sync_batch": (C.c_int, [_P, C.POINTER(C.c_int), C.c_int]),
    "slampp_hip_stream": (_P, [_P]),
    "slampp_hip_get_stats": (C.c_int, [_P, C.POINTER(Stats)]),
    "slampp_hip_get_reduced_stats": (C.c_int, [_P, C.POINTER(Stats)]),
    "slampp_hip_get_profile": (C.c_int, [_P, C.POINTER(PhaseTime), C.c_int, C.POINTER(C.c_int), C.c_int]),
    "slampp_hip_get_profile_reference_names": (C.c_int, [_P, C.POINTER(PhaseTime), C.c_int, C.POINTER(C.c_int)]),
    "slampp_hip_set_allreduce": (C.c_int, [_P, ALLREDUCE_FN, _P]),
    "slampp_hip_assembly_create": (C.c_int, [_P, C.POINTER(_P), C.c_int64, _P, _P, C.c_int]),
    "slampp_hip_assembly_destroy": (None, [_P]),
    "slampp_hip_assembly_get_info": (C.c_int, [_P, C.POINTER(AssemblyInfo)]),
    "slampp_hip_assemble_device_async": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int64, _P, _P, _P, _P, C.c_int]),
    "slampp_hip_assemble_sets_device_async": (C.c_int, [C.POINTER(EdgeSetPtrs), C.c_int, C.c_int64, _P, _P, _P, _P, C.c_int]),
    "slampp_hip_linearize_device_async": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P]),
    "slampp_hip_state_plus_device_async": (C.c_int, [_P, C.c_int, C.c_int64, C.c_int64, _P, _P, C.c_double, _P]),
    "slampp_hip_chi_squared_device_async": (C.c_int, [_P, _P, _P, _P, _P]),
    "slampp_hip_edge_errors_device_async": (C.c_int, [_P, C.c_int, _P, _P, _P, _P]),
    "slampp_hip_apply_damping_scalar_device_async": (C.c_int, [_P, _P, _P, C.c_double, C.c_int64, C.c_int64]),
    "slampp_hip_lm_initial_damping_device_async": (C.c_int, [C.POINTER(EdgeSetPtrs), C.c_int, C.c_double, _P]),
    "slampp_hip_lm_gain_device_async": (C.c_int, [_P, _P, _P, _P]),
    "slampp_hip_lm_decide_device_async": (C.c_int, [_P, _P, _P, C.c_int, _P, C.c_int64]),
    "slampp_hip_lm_commit_device_async": (C.c_int, [_P, _P, _P, _P]),
    "slampp_hip_lm_begin_device_async": (C.c_int, [C.POINTER(LmProblem), C.c_double, C.c_double, C.c_double, C.c_int, C.c_int]),
    "slampp_hip_lm_iterate_device_async": (C.c_int, [C.POINTER(LmProblem), C.c_int]),
    "slampp_hip_assembly_set_robust": (C.c_int, [_P, C.POINTER(Robust)]),
    "slampp_hip_assembly_robust_weights": (C.c_int, [_P, C.POINTER(_P)]),
    "slampp_hip_robust_weights_device_async": (C.c_int, [_P, _P, _P, _P]),
    "slampp_hip_robust_scale_device_async": (C.c_int, [_P, _P, _P, _P, _P]),
    "slampp_hip_robust_chi_squared_device_async": (C.c_int, [_P, _P, _P, _P]),
    "slampp_hip_get_plan": (C.c_int, [_P, C.POINTER(PlanView)]),
    "slampp_hip_plan_create": (C.c_int, [C.POINTER(_P), C.c_int64, _P, _P, _P, C.c_int, C.c_int, C.c_int]),
    "slampp_hip_plan_get": (C.c_int, [_P, C.POINTER(PlanView), C.POINTER(Stats)]),
    "slampp_hip_plan_destroy": (None, [_P]),
}

# the entry points that factor, drop the factor a handle keeps or change its structure: after any of them the factor an
# earlier call left is not that call's any more (values = NULL reuses of the covariance calls are counted too: harmless)
_FACTOR_CHANGING = frozenset(
    ["slampp_hip_free_memory", "slampp_hip_set_structure", "slampp_hip_analyze", "slampp_hip_factor_solve",
     "slampp_hip_factor_solve_device", "slampp_hip_factor_solve_device_async", "slampp_hip_factor_solve_batch_device_async",
     "slampp_hip_factorize", "slampp_hip_solve_marginal_poses", "slampp_hip_solve_marginal_poses_device_async",
     "slampp_hip_logdet", "slampp_hip_logdet_device_async", "slampp_hip_lm_iterate_device_async"] +
    [n for n in ABI if "marginal" in n and "poses" not in n])


class _FactorTrackingLib:
    """The library as one solver object calls it: every fetch of an entry point of _FACTOR_CHANGING counts ``generation``
    up, so that whoever remembers the generation of its own factorization (torch_solve) can tell whether the handle still
    holds that factor.  One place instead of a line in every wrapper method."""

    def __init__(self, lib):
        self._lib = lib
        self.generation = 0

    def __getattr__(self, name):
        if name in _FACTOR_CHANGING:
            self.generation += 1
        return getattr(self._lib, name)


_lib = None


def load_library() -> C.CDLL:
    """Loads libslampp_hip.so (built in-tree by ``__graft_entry__.build()``); raises if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)")
        try:
            # Python callers get their device memory from torch, which bundles its own HIP runtime: load that one
            # first, so that this library binds to it too -- two HIP runtimes in one process do not share the GPU
            # (whichever initialises second reports "no HIP GPUs")
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in ABI.items():
            fn = getattr(lib, name)   # AttributeError if the library does not export the symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


_PLAN_FIELDS = [("perm", "p_perm", np.int32, "n_bcols", 0), ("dim", "p_dim", np.int32, "n_bcols", 0),
                ("lptr", "p_lptr", np.int64, "n_bcols", 1), ("lrow", "p_lrow", np.int32, "l_blocks", 0),
                ("loff", "p_loff", np.int64, "l_blocks", 0), ("asrc", "p_asrc", np.int64, "l_blocks", 0),
                ("atrans", "p_atrans", np.int32, "l_blocks", 0), ("pptr", "p_pptr", np.int64, "l_blocks", 1),
                ("pa", "p_pa", np.int32, "n_pairs", 0), ("pb", "p_pb", np.int32, "n_pairs", 0),
                ("rptr", "p_rptr", np.int64, "n_bcols", 1), ("rblk", "p_rblk", np.int32, "n_row_entries", 0),
                ("stage_ptr", "p_stage_ptr", np.int32, "n_stages", 1),
                ("task_ptr", "p_task_ptr", np.int64, "n_tasks", 1),
                ("task_cols", "p_task_cols", np.int32, "n_task_cols", 0),
                ("dense_pos", "p_dense_pos", np.int32, "n_bcols", 0)]


def _fetch_plan(getter) -> dict:
    v = PlanView()
    getter(v)                                   # sizes
    out = {}
    for name, field, dt, size_field, extra in _PLAN_FIELDS:
        arr = np.zeros(getattr(v, size_field) + extra, dtype=dt)
        out[name] = arr
        setattr(v, field, arr.ctypes.data)
    getter(v)                                   # contents
    for f in ("n_bcols", "l_blocks", "n_pairs", "n_row_entries", "n_stages", "n_tasks", "l_values", "dense_dim"):
        out[f] = getattr(v, f)
    return out


def group_exchange_selftest(devices, exchange: int = 0, count: int = 1 << 16):
    """(status, name of the exchange used): the all-reduce of a multi-device handle by itself (slampp_hip_group_exchange_selftest)."""
    lib = load_library()
    ids = (C.c_int * len(devices))(*[int(d) for d in devices])
    buf = C.create_string_buffer(256)
    rc = lib.slampp_hip_group_exchange_selftest(ids, len(devices), int(exchange), int(count), buf, 256)
    return rc, buf.value.decode()


def landmark_shard_structure(lam, rank: int, world: int) -> dict:
    """The library's own shard splitter (slampp_hip_landmark_shard; host code, no GPU): structure arrays and value /
    right-hand side ranges of the landmark shard ``rank`` of ``world`` holds."""
    lib = load_library()
    cs = np.ascontiguousarray(lam.cumsum, dtype=np.int64)
    bp = np.ascontiguousarray(lam.bcol_ptr, dtype=np.int64)
    br = np.ascontiguousarray(lam.brow_idx, dtype=np.int32)
    v = ShardView()
    args = (lam.n_bcols, _ptr(cs), _ptr(bp), _ptr(br), int(lam.n_matrix_cut), int(rank), int(world))
    if lib.slampp_hip_landmark_shard(*args, C.byref(v)) != OK:
        raise ValueError("slampp_hip_landmark_shard refused the arguments")
    out = {"cumsum": np.zeros(v.n_bcols + 1, dtype=np.int64), "bcol_ptr": np.zeros(v.n_bcols + 1, dtype=np.int64),
           "brow_idx": np.zeros(v.n_blocks, dtype=np.int32)}
    v.p_bcol_cumsum, v.p_bcol_ptr, v.p_brow_idx = (out[k].ctypes.data for k in ("cumsum", "bcol_ptr", "brow_idx"))
    if lib.slampp_hip_landmark_shard(*args, C.byref(v)) != OK:
        raise ValueError("slampp_hip_landmark_shard refused the arguments")
    for k, _ in ShardView._fields_[:10]:
        out[k] = int(getattr(v, k))
    return out


def host_plan(lam, leaf_size: int = 0, subtree_size: int = 0, dense_top_nb: int = -1):
    """Ordering + symbolic analysis + schedule on the host only (no GPU): (plan dict, stats dict).
    ``dense_top_nb`` < 0 = the library default, 0 = no dense top."""
    lib = load_library()
    h = C.c_void_p()
    cs = np.ascontiguousarray(lam.cumsum, dtype=np.int64)
    bp = np.ascontiguousarray(lam.bcol_ptr, dtype=np.int64)
    br = np.ascontiguousarray(lam.brow_idx, dtype=np.int32)
    rc = lib.slampp_hip_plan_create(C.byref(h), lam.n_bcols, _ptr(cs), _ptr(bp), _ptr(br),
                                    leaf_size, subtree_size, dense_top_nb)
    if rc != OK:
        raise ValueError(f"slampp_hip_plan_create failed ({rc})")
    try:
        st = Stats()

        def getter(v):
            if lib.slampp_hip_plan_get(h, C.byref(v), C.byref(st)) != OK:
                raise RuntimeError("slampp_hip_plan_get failed")
        plan = _fetch_plan(getter)
        return plan, st.as_dict()
    finally:
        lib.slampp_hip_plan_destroy(h)


class _SolverBase:
    """Shared plumbing: handle life cycle, structure caching, status -> exception mapping."""

    _mode = MODE_SPARSE

    def __init__(self, device: int = 0, devices=None, **options):
        """``devices``: a list of HIP device ordinals -- one handle over several GPUs of this process
        (slampp_hip_create_multi): a BA system is cut into landmark shards, one per listed device, and the reduced camera
        system is summed inside the library (RCCL, or peer pointers); pose graphs run on ``devices[0]``."""
        self._lib = _FactorTrackingLib(load_library())
        self.n_backward_refactorizations = 0     # torch_solve: backward passes that had to factor again
        self._h = C.c_void_p()
        self._devices = None if devices is None else [int(d) for d in devices]
        if self._devices is not None:
            if not self._devices:
                raise ValueError("devices must name at least one device")
            ids = (C.c_int * len(self._devices))(*self._devices)
            rc = self._lib.slampp_hip_create_multi(C.byref(self._h), ids, len(self._devices))
            device = self._devices[0]
        else:
            rc = self._lib.slampp_hip_create(C.byref(self._h), int(device))
        if rc == ERR_INVALID:
            self._h = None
            raise ValueError(f"slampp_hip_create_multi(devices={self._devices}) refused the device list" if self._devices is not None
                             else f"slampp_hip_create(device={device}) refused the device ordinal")
        if rc != OK:
            self._h = None
            raise RuntimeError(f"slampp_hip_create(device={device}) failed ({rc}): no usable HIP device")
        self._device = int(device)
        self._options = dict(options)
        self._options_now = dict(options)        # ... and what set_option() has changed since (copies do not carry it)
        for k, v in options.items():
            self._check(self._lib.slampp_hip_set_option(self._h, k.encode(), int(v)))
        self._structure_key = None
        self._analyzed = False
        self._keepalive = None
        self.times = Times()

    # copies do not carry state, as in the reference (LinearSolver_CholMod.h:163-167,
    # NonlinearSolver_Base.h:400,438), but they do keep the configuration
    def __copy__(self):
        return type(self)(**self._ctor_args())

    def _ctor_args(self):
        return dict(self._options, device=self._device, devices=self._devices)

    def group_info(self) -> dict:
        """Members in use, their landmark ranges and the exchange of a handle made with ``devices=[...]``
        (``{"members": 0, ...}`` while the handle is not solving with shards)."""
        n = C.c_int(0)
        name = C.c_char_p()
        bounds = np.zeros(17, dtype=np.int64)
        self._check(self._lib.slampp_hip_group_info(self._h, C.byref(n), _ptr(bounds), 16, C.byref(name)))
        return {"members": n.value, "point_bounds": bounds[:n.value + 1].tolist() if n.value else [],
                "exchange": (name.value or b"").decode()}

    def exchange_count(self) -> int:
        """Exchanges the members of a device group have gone into (slampp_hip_group_exchange_count): all of them or none."""
        n = C.c_int64(0)
        self._check(self._lib.slampp_hip_group_exchange_count(self._h, C.byref(n)))
        return int(n.value)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.slampp_hip_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _error(self) -> str:
        return (self._lib.slampp_hip_last_error(self._h) or b"").decode()

    def _check(self, rc: int) -> bool:
        if rc == OK:
            return True
        if rc == NOT_POSDEF:
            return False
        if rc == ERR_ALLOC:
            raise MemoryError(self._error())
        if rc == ERR_INVALID:
            raise ValueError(self._error())
        if rc == ERR_UNSUPPORTED:
            raise NotImplementedError(self._error())
        raise RuntimeError(self._error())

    def Free_Memory(self) -> None:
        self._check(self._lib.slampp_hip_free_memory(self._h))
        self._structure_key = None
        self._analyzed = False

    def Clear_SymbolicDecomposition(self) -> None:
        """LinearSolverTags.h:112-120: the block structure is about to change."""
        self._structure_key = None
        self._analyzed = False

    def _key(self, lam):
        """Identity of the block structure.  The same array objects as last time (what an iteration loop passes) are not
        hashed again -- 10^6 indices per call --, but they are not trusted blindly either: a caller that edits the index
        arrays in place (same objects, same shapes) would otherwise have the old analysis applied to a new pattern, a wrong
        answer without an error.  So the fast path compares a strided sample of each array (1024 entries + both ends)
        with what was there when the key was taken; a system that carries a ``structure_version`` counter is keyed on that
        as well.  An edit that misses every sampled entry still needs ``Clear_SymbolicDecomposition()``, as in the
        reference (LinearSolverTags.h:112-120)."""
        arrays = (lam.bcol_ptr, lam.brow_idx, lam.cumsum)
        ident = tuple(id(a) for a in arrays) + (getattr(lam, "structure_version", None),)
        if getattr(self, "_key_ident", None) == ident and all(a is b for a, b in zip(self._key_arrays, arrays)) and \
                all(np.array_equal(self._sample(a), s) for a, s in zip(arrays, self._key_samples)):
            return self._key_value
        key = (lam.n_bcols, lam.n_blocks, int(lam.cumsum[-1]),
               _hash_array(lam.bcol_ptr), _hash_array(lam.brow_idx), _hash_array(lam.cumsum))
        self._key_ident, self._key_arrays, self._key_value = ident, arrays, key
        self._key_samples = tuple(self._sample(a).copy() for a in arrays)
        return key

    @staticmethod
    def _sample(a: np.ndarray) -> np.ndarray:
        n = a.shape[0]
        if n <= 2048:
            return a
        return np.concatenate([a[::max(n // 1024, 1)], a[-2:]])

    def _n_matrix_cut(self, lam) -> int:
        return 0

    def SymbolicDecomposition_Blocky(self, lam) -> bool:
        cs = np.ascontiguousarray(lam.cumsum, dtype=np.int64)
        bp = np.ascontiguousarray(lam.bcol_ptr, dtype=np.int64)
        br = np.ascontiguousarray(lam.brow_idx, dtype=np.int32)
        self._check(self._lib.slampp_hip_set_structure(self._h, lam.n_bcols, _ptr(cs), _ptr(bp), _ptr(br)))
        self._check(self._lib.slampp_hip_analyze(self._h, self._mode, self._n_matrix_cut(lam)))
        self._structure_key = self._key(lam)
        self._n_values = int(lam.values.shape[0])
        self._analyzed = True
        return True

    def Solve_PosDef_Blocky(self, lam, eta: np.ndarray) -> bool:
        """Reuses ordering / symbolic analysis while the block structure is unchanged
        (LinearSolverTags.h:130-134).  ``eta``: rhs on entry, solution on return."""
        if eta.dtype != np.float64 or not eta.flags.c_contiguous or eta.shape != (lam.n_scalars,):
            raise ValueError("eta must be a contiguous float64 vector of the system's dimension")
        if not self._analyzed or self._structure_key != self._key(lam):
            self._check(self._lib.slampp_hip_set_option(self._h, b"staging_ahead", 1))   # host arrays: the staging beside the analysis
            self.SymbolicDecomposition_Blocky(lam)
        vals = np.ascontiguousarray(lam.values, dtype=np.float64)
        if vals.shape != (self._n_values,):
            raise ValueError("lam.values does not match the block structure")
        return self._check(self._lib.slampp_hip_factor_solve(self._h, _ptr(vals), _ptr(eta), C.byref(self.times)))

    def Solve_PosDef(self, lam, eta: np.ndarray) -> bool:
        """Cold solve: ordering + symbolic + numeric (LinearSolver_CholMod.cpp:264-358)."""
        self.Clear_SymbolicDecomposition()
        return self.Solve_PosDef_Blocky(lam, eta)

    def Solve_Again(self, eta: np.ndarray) -> bool:
        """Another right-hand side with the factor the last solve left behind (cholmod_solve on a kept factor,
        LinearSolver_CholMod.cpp:322-347).  Schur mode: needs the option ``schur_keep=1`` (or a Schur covariance call
        before it), which keeps W, C^-1 and the reduced system's factor; NotImplementedError without."""
        if self._structure_key is None or not self._analyzed:
            raise ValueError("Solve_Again: there is no factorization")
        n_scalars = self._structure_key[2]
        if eta.dtype != np.float64 or not eta.flags.c_contiguous or eta.shape != (n_scalars,):
            raise ValueError("eta must be a contiguous float64 vector of the system's dimension")
        return self._check(self._lib.slampp_hip_solve_again(self._h, _ptr(eta)))

    def Solve_Columns(self, B: np.ndarray) -> bool:
        """k right-hand sides with the factor the last solve left behind, in one call (slampp_hip_solve_columns: cholmod_solve
        with a dense B of several columns).  ``B``: a C-contiguous float64 ``(k, n_scalars)`` array, 1 <= k <= 256, row c =
        right-hand side c on entry and its solution on return.  Valid where Solve_Again is."""
        if self._structure_key is None or not self._analyzed:
            raise ValueError("Solve_Columns: there is no factorization")
        n_scalars = self._structure_key[2]
        if (not isinstance(B, np.ndarray) or B.dtype != np.float64 or not B.flags.c_contiguous or B.ndim != 2
                or B.shape[1] != n_scalars or not 1 <= B.shape[0] <= SOLVE_MAX_COLUMNS):
            raise ValueError(f"B must be a C-contiguous float64 array of the shape (k, n_scalars), 1 <= k <= {SOLVE_MAX_COLUMNS}")
        return self._check(self._lib.slampp_hip_solve_columns(self._h, _ptr(B), n_scalars, int(B.shape[0])))

    def Solve_Half_Columns(self, B: np.ndarray, half: int) -> bool:
        """One of the two substitutions of Solve_Columns alone (slampp_hip_solve_half_columns: cholmod_solve with CHOLMOD_P +
        CHOLMOD_L, or with CHOLMOD_Lt + CHOLMOD_Pt), on a C-contiguous float64 ``(k, n_scalars)`` array as Solve_Columns takes.
        ``half=HALF_FORWARD``: row c holds b in the caller's scalar order on entry and ``y = L^-1 P b`` in the factor's order
        (the block permutation of factor_structure()) on return; ``half=HALF_BACKWARD``: y in the factor's order on entry,
        ``x = P^T L^-T y`` in the caller's order on return.  Sparse mode with block columns of at most 8; NotImplementedError
        in Schur mode (the factor there is a block factor over the landmarks' own Cholesky factors) and for wider blocks."""
        if self._structure_key is None or not self._analyzed:
            raise ValueError("Solve_Half_Columns: there is no factorization")
        n_scalars = self._structure_key[2]
        if (not isinstance(B, np.ndarray) or B.dtype != np.float64 or not B.flags.c_contiguous or B.ndim != 2
                or B.shape[1] != n_scalars or not 1 <= B.shape[0] <= SOLVE_MAX_COLUMNS):
            raise ValueError(f"B must be a C-contiguous float64 array of the shape (k, n_scalars), 1 <= k <= {SOLVE_MAX_COLUMNS}")
        return self._check(self._lib.slampp_hip_solve_half_columns(self._h, int(half), _ptr(B), n_scalars, int(B.shape[0])))

    def Log_Determinant(self, lam, reuse_factor: bool = False) -> float:
        """log det Lambda = 2 sum log L_ii from the Cholesky factor on the device (slampp_hip_logdet).  ``reuse_factor=False``:
        analyzes a new structure, factors ``lam.values`` and leaves the handle as Solve_PosDef_Blocky leaves it (Solve_Again
        is valid afterwards).  ``reuse_factor=True``: nothing is factored, the factor the last solve left is read
        (ValueError if there is none; Schur mode: option ``schur_keep=1``, and ``lam.values`` must be the values that solve
        factored).  A matrix that is not positive definite has no log-determinant: as Solve_PosDef_Blocky answers False
        there without raising, this returns NaN without raising."""
        if reuse_factor:
            if not self._analyzed or self._structure_key != self._key(lam):
                raise ValueError("Log_Determinant: there is no factorization of this structure to reuse")
        elif not self._analyzed or self._structure_key != self._key(lam):
            self._check(self._lib.slampp_hip_set_option(self._h, b"staging_ahead", 1))   # host arrays: the staging beside the analysis
            self.SymbolicDecomposition_Blocky(lam)
        vals = np.ascontiguousarray(lam.values, dtype=np.float64)
        if vals.shape != (self._n_values,):
            raise ValueError("lam.values does not match the block structure")
        out = C.c_double(float("nan"))
        if not self._check(self._lib.slampp_hip_logdet(self._h, _ptr(vals), int(bool(reuse_factor)), C.byref(out))):
            return float("nan")
        return float(out.value)

    def _set_structure(self, lam) -> None:
        """The block structure alone (slampp_hip_set_structure): what the product needs; a solve analyzes it later."""
        cs = np.ascontiguousarray(lam.cumsum, dtype=np.int64)
        bp = np.ascontiguousarray(lam.bcol_ptr, dtype=np.int64)
        br = np.ascontiguousarray(lam.brow_idx, dtype=np.int32)
        self._check(self._lib.slampp_hip_set_structure(self._h, lam.n_bcols, _ptr(cs), _ptr(bp), _ptr(br)))
        self._structure_key = self._key(lam)
        self._n_values = int(lam.values.shape[0])
        self._analyzed = False

    def Multiply(self, lam, x: np.ndarray, y: np.ndarray = None, alpha: float = 1.0, beta: float = 0.0) -> np.ndarray:
        """y = alpha Lambda x + beta y for the symmetric Lambda whose upper blocks ``lam`` stores (slampp_hip_multiply);
        returns y (a new vector where none is given, which needs beta = 0).  No analysis is needed."""
        if self._structure_key is None or self._structure_key != self._key(lam):
            self._set_structure(lam)
        n = int(lam.cumsum[-1])
        if y is None:
            if beta != 0:
                raise ValueError("Multiply: beta != 0 needs a y")
            y = np.empty(n, dtype=np.float64)
        for v in (x, y):
            if v.dtype != np.float64 or not v.flags.c_contiguous or v.shape != (n,):
                raise ValueError("x and y must be contiguous float64 vectors of the system's dimension")
        vals = np.ascontiguousarray(lam.values, dtype=np.float64)
        if vals.shape != (self._n_values,):
            raise ValueError("lam.values does not match the block structure")
        self._check(self._lib.slampp_hip_multiply(self._h, _ptr(vals), _ptr(x), _ptr(y), float(alpha), float(beta)))
        return y

    def Pattern_Outer(self, lam, a: np.ndarray, b: np.ndarray, out: np.ndarray = None, alpha: float = 1.0,
                      beta: float = 0.0) -> np.ndarray:
        """out = alpha P(a, b) + beta out on the block pattern of ``lam`` (slampp_hip_pattern_outer): alpha (a_r b_c^T +
        b_r a_c^T) at every stored block r < c, alpha a_r b_r^T at every diagonal block -- the adjoint of Multiply with respect
        to ``lam.values``.  Returns out, shaped like ``lam.values`` (a new array where none is given, which needs beta = 0).
        No analysis is needed."""
        if self._structure_key is None or self._structure_key != self._key(lam):
            self._set_structure(lam)
        n = int(lam.cumsum[-1])
        if out is None:
            if beta != 0:
                raise ValueError("Pattern_Outer: beta != 0 needs an out")
            out = np.empty(self._n_values, dtype=np.float64)
        for v in (a, b):
            if v.dtype != np.float64 or not v.flags.c_contiguous or v.shape != (n,):
                raise ValueError("a and b must be contiguous float64 vectors of the system's dimension")
        if out.dtype != np.float64 or not out.flags.c_contiguous or out.shape != (self._n_values,):
            raise ValueError("out must be a contiguous float64 vector shaped like lam.values")
        self._check(self._lib.slampp_hip_pattern_outer(self._h, _ptr(a), _ptr(b), _ptr(out), float(alpha), float(beta)))
        return out

    def Refine(self, lam, eta: np.ndarray, x: np.ndarray, n_steps: int = 2) -> np.ndarray:
        """``n_steps`` of iterative refinement of ``x`` (in place) with the kept factor (slampp_hip_refine): r = eta - Lambda x,
        d = Solve_Again(r), x += d, where a step that does not at least halve max|eta - Lambda x| is taken back and ends the
        refinement.  Returns the n_steps + 1 residual norms max|eta - Lambda x_k| of the x held before every step and of
        the x returned; they never grow.  ValueError without a valid kept factor (Schur mode: option ``schur_keep=1``)."""
        n = int(lam.cumsum[-1])
        for v in (eta, x):
            if v.dtype != np.float64 or not v.flags.c_contiguous or v.shape != (n,):
                raise ValueError("eta and x must be contiguous float64 vectors of the system's dimension")
        vals = np.ascontiguousarray(lam.values, dtype=np.float64)
        if self._structure_key is None or self._structure_key != self._key(lam) or vals.shape != (self._n_values,):
            raise ValueError("Refine: lam is not the system this handle factorized")
        resid = np.zeros(max(int(n_steps), 0) + 1, dtype=np.float64)
        self._check(self._lib.slampp_hip_refine(self._h, _ptr(vals), _ptr(eta), _ptr(x), int(n_steps), _ptr(resid)))
        return resid

    def host_staging(self):
        """(values, rhs): numpy views of the library's pinned staging for the current structure -- filling these and
        passing them to Solve_PosDef_Blocky spares the transfers a staging pass (slampp_hip_host_staging)."""
        pv, pr = C.c_void_p(), C.c_void_p()
        self._check(self._lib.slampp_hip_host_staging(self._h, C.byref(pv), C.byref(pr)))
        st = Stats()
        self._check(self._lib.slampp_hip_get_stats(self._h, C.byref(st)))
        n_values = int(self._n_values)
        values = np.ctypeslib.as_array(C.cast(pv, C.POINTER(C.c_double)), shape=(n_values,))
        rhs = np.ctypeslib.as_array(C.cast(pr, C.POINTER(C.c_double)), shape=(int(st.n_scalars),))
        return values, rhs

    def factor_structure(self) -> dict:
        """Block structure of the factor slampp_hip_factorize hands back, over the caller's block columns
        (slampp_hip_factor_structure): ``perm``, ``dim``, ``lptr``, ``lrow``, ``loff``, ``l_values``."""
        n, nb, nv = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._check(self._lib.slampp_hip_factor_structure(self._h, C.byref(n), C.byref(nb), C.byref(nv), None, None, None, None, None))
        out = {"perm": np.zeros(n.value, dtype=np.int32), "dim": np.zeros(n.value, dtype=np.int32),
               "lptr": np.zeros(n.value + 1, dtype=np.int64), "lrow": np.zeros(nb.value, dtype=np.int32),
               "loff": np.zeros(nb.value, dtype=np.int64)}
        self._check(self._lib.slampp_hip_factor_structure(self._h, C.byref(n), C.byref(nb), C.byref(nv), _ptr(out["perm"]), _ptr(out["dim"]),
                                                          _ptr(out["lptr"]), _ptr(out["lrow"]), _ptr(out["loff"])))
        out["l_values"] = int(nv.value)
        return out

    def factorize(self, lam):
        """Numeric factor only (sparse mode): ``(ok, structure, l_values)`` -- the lower factor of the permuted Lambda in
        block-CSC over the caller's block columns (``structure['lptr']``, ``['lrow']``, ``['loff']``, ``['perm']``, ``['dim']``:
        factor_structure()); a dense top's columns and the pieces of block columns wider than 8 come back in that layout too."""
        if not self._analyzed or self._structure_key != self._key(lam):
            self.SymbolicDecomposition_Blocky(lam)
        plan = self.factor_structure()
        vals = np.ascontiguousarray(lam.values, dtype=np.float64)
        out = np.zeros(int(plan["l_values"]))
        ok = self._check(self._lib.slampp_hip_factorize(self._h, _ptr(vals), _ptr(out)))
        return ok, plan, out

    def stats(self) -> dict:
        st = Stats()
        self._check(self._lib.slampp_hip_get_stats(self._h, C.byref(st)))
        return st.as_dict()

    def reduced_stats(self) -> dict:
        """Schur mode, after a solve: stats of the inner sparse solver of the reduced camera system (all zero: dense)."""
        st = Stats()
        self._check(self._lib.slampp_hip_get_reduced_stats(self._h, C.byref(st)))
        return st.as_dict()

    def set_option(self, name: str, value: int) -> None:
        self._check(self._lib.slampp_hip_set_option(self._h, name.encode(), int(value)))
        self._options_now[name] = int(value)

    @property
    def factor_generation(self) -> int:
        """Counts up with every call through this object that factors, drops the kept factor or changes the structure."""
        return self._lib.generation

    def profile(self, reset: bool = False) -> dict:
        """{phase: (count, total_ms)} measured with HIP events on the solver's stream (option profile=1)."""
        buf = (PhaseTime * 32)()
        n = C.c_int(0)
        self._check(self._lib.slampp_hip_get_profile(self._h, buf, 32, C.byref(n), int(reset)))
        return {buf[i].name.decode(): (int(buf[i].n_count), float(buf[i].f_total_ms)) for i in range(min(n.value, 32))}

    def profile_reference_names(self) -> dict:
        """The same totals under the names the reference prints with __SCHUR_PROFILING (LinearSolver_Schur.h:1895-1912) /
        CHOLMOD's numeric phases: {name: (count, total_ms)}, in the reference's order (slampp_hip_get_profile_reference_names)."""
        buf = (PhaseTime * 16)()
        n = C.c_int(0)
        self._check(self._lib.slampp_hip_get_profile_reference_names(self._h, buf, 16, C.byref(n)))
        return {buf[i].name.decode(): (int(buf[i].n_count), float(buf[i].f_total_ms)) for i in range(min(n.value, 16))}

    def plan(self) -> dict:
        def getter(v):
            self._check(self._lib.slampp_hip_get_plan(self._h, C.byref(v)))
        return _fetch_plan(getter)

    # ---- device-resident entry points (bench.py; torch only provides the memory) ----
    def factor_solve_device(self, values_ptr: int, rhs_ptr: int) -> bool:
        return self._check(self._lib.slampp_hip_factor_solve_device(self._h, values_ptr, rhs_ptr, C.byref(self.times)))

    def factor_solve_device_async(self, values_ptr: int, rhs_ptr: int) -> None:
        self._check(self._lib.slampp_hip_factor_solve_device_async(self._h, values_ptr, rhs_ptr))

    def factor_solve_batch_device_async(self, n_batch: int, values_ptr: int, values_stride: int, rhs_ptr: int, rhs_stride: int) -> None:
        """K value sets of the analyzed structure in one pass of launches (slampp_hip_factor_solve_batch_device_async): member k
        reads values_ptr + 8 k values_stride and overwrites rhs_ptr + 8 k rhs_stride (strides in doubles)."""
        self._check(self._lib.slampp_hip_factor_solve_batch_device_async(self._h, int(n_batch), values_ptr, int(values_stride), rhs_ptr, int(rhs_stride)))

    def sync_batch(self, n_batch: int):
        """Waits for the batches enqueued so far; one bool per member: False = that member's matrix is not positive definite."""
        st = (C.c_int * int(n_batch))()
        self._check(self._lib.slampp_hip_sync_batch(self._h, st, int(n_batch)))
        return [v == 0 for v in st]

    def sync(self) -> bool:
        return self._check(self._lib.slampp_hip_sync(self._h))

    def solve_again_device(self, rhs_ptr: int) -> None:
        """Another right-hand side with the kept factor, device-resident and enqueue-only, in both modes
        (slampp_hip_solve_again_device_async; Schur mode: option ``schur_keep=1``)."""
        self._check(self._lib.slampp_hip_solve_again_device_async(self._h, rhs_ptr))

    def solve_columns_device(self, rhs_ptr: int, ld: int, k: int) -> None:
        """k right-hand sides with the kept factor in one call, device-resident and enqueue-only, in both modes
        (slampp_hip_solve_columns_device_async): column c is the n_scalars doubles at rhs_ptr + 8 c ld; valid where
        solve_again_device is."""
        self._check(self._lib.slampp_hip_solve_columns_device_async(self._h, rhs_ptr or None, int(ld), int(k)))

    def solve_half_columns_device(self, rhs_ptr: int, ld: int, k: int, half: int) -> None:
        """One of the two substitutions of solve_columns_device alone, device-resident and enqueue-only
        (slampp_hip_solve_half_columns_device_async): ``half=HALF_FORWARD`` turns column c, b in the caller's scalar order, into
        ``L^-1 P b`` in the factor's order; ``half=HALF_BACKWARD`` turns y in the factor's order into ``P^T L^-T y`` in the
        caller's.  One after the other they give solve_columns_device's bits.  Sparse mode, block columns of at most 8."""
        self._check(self._lib.slampp_hip_solve_half_columns_device_async(self._h, int(half), rhs_ptr or None, int(ld), int(k)))

    def gram_device(self, a_ptr: int, lda: int, ka: int, b_ptr: int, ldb: int, kb: int, n_rows: int, out_ptr: int, ldo: int) -> None:
        """out(i, j) = a_i . b_j over n_rows device-resident doubles, in a fixed order (slampp_hip_gram_device_async): a_i at
        a_ptr + 8 i lda, b_j at b_ptr + 8 j ldb, out(i, j) at out_ptr + 8 (i + j ldo); ka, kb <= GRAM_MAX_COLUMNS.
        Enqueue-only; any handle."""
        self._check(self._lib.slampp_hip_gram_device_async(self._h, a_ptr or None, int(lda), int(ka), b_ptr or None, int(ldb), int(kb),
                                                           int(n_rows), out_ptr or None, int(ldo)))

    def multiply_device(self, values_ptr: int, x_ptr: int, y_ptr: int, alpha: float = 1.0, beta: float = 0.0) -> None:
        """y = alpha Lambda x + beta y on device-resident arrays, enqueue-only (slampp_hip_multiply_device_async); the
        structure is the one last given to the handle."""
        self._check(self._lib.slampp_hip_multiply_device_async(self._h, values_ptr, x_ptr, y_ptr, float(alpha), float(beta)))

    def pattern_outer_device(self, a_ptr: int, b_ptr: int, out_ptr: int, alpha: float = 1.0, beta: float = 0.0) -> None:
        """out = alpha P(a, b) + beta out on device-resident arrays, enqueue-only (slampp_hip_pattern_outer_device_async);
        the structure is the one last given to the handle, out has the length of its packed values."""
        self._check(self._lib.slampp_hip_pattern_outer_device_async(self._h, a_ptr or None, b_ptr or None, out_ptr or None,
                                                                    float(alpha), float(beta)))

    def pattern_outer_batch_device(self, n_batch: int, a_ptr: int, a_stride: int, b_ptr: int, b_stride: int, out_ptr: int,
                                   out_stride: int, alpha: float = 1.0, beta: float = 0.0) -> None:
        """The same for n_batch members in one launch (slampp_hip_pattern_outer_batch_device_async): member m reads
        a_ptr + 8 m a_stride and b_ptr + 8 m b_stride and writes out_ptr + 8 m out_stride (strides in doubles)."""
        self._check(self._lib.slampp_hip_pattern_outer_batch_device_async(
            self._h, int(n_batch), a_ptr or None, int(a_stride), b_ptr or None, int(b_stride), out_ptr or None, int(out_stride),
            float(alpha), float(beta)))

    def pattern_outer_sum_device(self, n_terms: int, a_ptr: int, a_stride: int, b_ptr: int, b_stride: int, out_ptr: int,
                                 alpha: float = 1.0, beta: float = 0.0) -> None:
        """out = alpha sum_k P(a_k, b_k) + beta out in one launch (slampp_hip_pattern_outer_sum_device_async): term k reads
        a_ptr + 8 k a_stride and b_ptr + 8 k b_stride (strides in doubles), out is written once."""
        self._check(self._lib.slampp_hip_pattern_outer_sum_device_async(
            self._h, int(n_terms), a_ptr or None, int(a_stride), b_ptr or None, int(b_stride), out_ptr or None,
            float(alpha), float(beta)))

    def dot_device(self, a_ptr: int, b_ptr: int, n: int, out_ptr: int) -> None:
        """*out = a . b over n device-resident doubles, in a fixed order (slampp_hip_dot_device_async)."""
        self._check(self._lib.slampp_hip_dot_device_async(self._h, a_ptr, b_ptr, int(n), out_ptr))

    def refine_device(self, values_ptr: int, eta_ptr: int, x_ptr: int, n_steps: int, resid_ptr: int = 0) -> None:
        """Iterative refinement on device-resident arrays, enqueue-only (slampp_hip_refine_device_async); ``resid_ptr``:
        n_steps + 1 doubles, or 0."""
        self._check(self._lib.slampp_hip_refine_device_async(self._h, values_ptr, eta_ptr, x_ptr, int(n_steps), resid_ptr or None))

    def logdet_device(self, values_ptr: int, out_ptr: int, reuse_factor: bool = False) -> None:
        """*out = log det Lambda from the Cholesky factor, device-resident and enqueue-only (slampp_hip_logdet_device_async).
        ``reuse_factor=False``: the values are factored first and the handle is left as factor_solve_device_async leaves
        it; ``True``: the factor in place is read (sparse mode: wherever solve_again_device is valid, ``values_ptr`` may be
        0; Schur mode: after a solve with ``schur_keep=1``, and the values are still needed for the landmark blocks).  NaN is
        written where the matrix is not positive definite, which ``sync()`` then reports."""
        self._check(self._lib.slampp_hip_logdet_device_async(self._h, values_ptr or None, int(bool(reuse_factor)), out_ptr or None))

    def marginals_pattern_device(self, values_ptr: int, out_ptr: int) -> None:
        """Lambda^-1 at every stored block of Lambda on device-resident arrays, enqueue-only: the class's pattern entry point
        (slampp_hip_marginals_pattern_device_async / slampp_hip_schur_marginals_pattern_device_async); ``out_ptr``: as many
        doubles as the packed values.  Factors the values (Schur mode: ``values_ptr`` = 0 reuses what the previous Schur
        covariance call left)."""
        self._check(getattr(self._lib, self._covariance_entries[0] + "_device_async")(self._h, values_ptr or None, out_ptr or None))

    def apply_damping_device_async(self, values_ptr: int, f_alpha: float, n_first_vertex: int, n_last_vertex: int) -> None:
        """ApplyDamping of the reference's LM solver (NonlinearSolver_Lambda_LM.h:228-239) on device-resident values."""
        self._check(self._lib.slampp_hip_apply_damping_device_async(self._h, values_ptr, float(f_alpha), int(n_first_vertex),
                                                                    int(n_last_vertex)))

    def State_Plus_device(self, vertex_type: int, first: int, last: int, state_ptr: int, dx_ptr: int, out_ptr: int,
                          scale: float = 1.0) -> None:
        """out = state (+) scale dx on block columns [first, last), on the manifold of ``vertex_type`` (VERTEX_*): the
        reference's Operator_Plus over the vertex pool, ``scale=-1`` its Operator_Minus (slampp_hip_state_plus_device_async).
        ``out_ptr`` may be ``state_ptr``; block columns outside the range are not written.  Needs the structure only: set it
        with SymbolicDecomposition_Blocky, or create a CLambdaAssembly_HIP first.  Enqueue-only."""
        self._check(self._lib.slampp_hip_state_plus_device_async(self._h, int(vertex_type), int(first), int(last), state_ptr or None,
                                                                 dx_ptr or None, float(scale), out_ptr or None))

    def stream(self) -> int:
        return int(self._lib.slampp_hip_stream(self._h) or 0)

    def set_allreduce(self, fn) -> None:
        """fn(dev_ptr:int, count:int, stream:int) -> int; kept alive by the solver."""
        if fn is None:
            self._keepalive = None
            self._check(self._lib.slampp_hip_set_allreduce(self._h, C.cast(None, ALLREDUCE_FN), None))
            return

        def tramp(_ctx, p, n, s):
            try:
                return int(fn(int(p or 0), int(n), int(s or 0)))
            except Exception:      # never unwind through C
                return 1
        self._keepalive = ALLREDUCE_FN(tramp)
        self._check(self._lib.slampp_hip_set_allreduce(self._h, self._keepalive, None))


    # ---- covariances: one implementation for both classes; ``_covariance_entries`` names the class's C entry points
    # (pattern, columns, blocks) ----

    def _covariance_values(self, lam, reuse_factor: bool, who: str):
        """What a covariance call passes as values: ``None`` to reuse the factor in place (ValueError if this structure
        has none), else the contiguous ``lam.values``, after the analysis of a new structure."""
        if reuse_factor:
            if not self._analyzed or self._structure_key != self._key(lam):
                raise ValueError(f"{who}: there is no factorization of this structure to reuse")
            return None
        if not self._analyzed or self._structure_key != self._key(lam):
            self.SymbolicDecomposition_Blocky(lam)
        vals = np.ascontiguousarray(lam.values, dtype=np.float64)
        if vals.shape != (self._n_values,):
            raise ValueError("lam.values does not match the block structure")
        return vals

    def _marginals_pattern(self, lam, reuse_factor: bool = False) -> np.ndarray:
        """Lambda^-1 at every stored block of Lambda: an array shaped like ``lam.values`` (same block order, each block
        column-major), as CMarginals::Calculate_DenseMarginals_Recurrent_FBS gives it on a factor's pattern
        (Marginals.h:1696) -- on Lambda's pattern here, which is the same under every ordering.
        CLinearSolver_Schur_HIP: camera blocks, camera-landmark observation blocks, landmark diagonal blocks; it also takes
        ``reuse_factor``: the reduced system's factor, C^-1 and W the previous Marginals_Pattern / Marginal_Columns call
        left are used (ValueError if anything else factored since)."""
        vals = self._covariance_values(lam, reuse_factor, "Marginals_Pattern")
        out = np.empty(self._n_values, dtype=np.float64)
        if not self._check(getattr(self._lib, self._covariance_entries[0])(self._h, _ptr(vals) if vals is not None else None,
                                                                          _ptr(out))):
            raise ArithmeticError("Marginals_Pattern: the system is not positive definite")
        return out

    def Marginal_Columns(self, lam, bcols, reuse_factor: bool = False) -> np.ndarray:
        """Whole block columns ``bcols`` of Lambda^-1 (Schur mode: cameras and landmarks in any mix), shape (n_scalars, k),
        k = the sum of their dimensions, in the listed order (the reference's mpart_Column / mpart_LastColumn,
        IncrementalPolicy.h:366-372).  ``reuse_factor``: the factor the last solve or covariance call left in place is
        used (Schur mode: what the previous Marginals_Pattern / Marginal_Columns call left), ``lam.values`` are not
        factored again."""
        cols = np.ascontiguousarray(np.atleast_1d(np.asarray(bcols, dtype=np.int64)))
        vals = self._covariance_values(lam, reuse_factor, "Marginal_Columns")
        dims = np.diff(np.asarray(lam.cumsum, dtype=np.int64))
        k = int(dims[cols].sum()) if cols.size and cols.min() >= 0 and cols.max() < len(dims) else 0
        out = np.empty((max(k, 1), int(lam.cumsum[-1])), dtype=np.float64)   # column-major (n_scalars, k) = row-major (k, n_scalars)
        if not self._check(getattr(self._lib, self._covariance_entries[1])(self._h, _ptr(vals) if vals is not None else None,
                                                                          int(cols.size), _ptr(cols), _ptr(out))):
            raise ArithmeticError("Marginal_Columns: the system is not positive definite")
        return out[:k].T

    def Marginal_Blocks(self, lam, pairs, reuse_factor: bool = False) -> list:
        """Blocks of Lambda^-1 at arbitrary pairs ``(r, c)`` of block columns, inside Lambda's pattern or outside it: a list
        of d_r x d_c arrays in the listed order (what g2o's computeMarginals(spinv, blockIndices) answers).  No whole columns
        are formed.  ``reuse_factor``: as for the class's Marginal_Columns.
        CLinearSolver_HIP (slampp_hip_marginal_blocks): forward substitutions over the two columns' elimination-tree paths.
        CLinearSolver_Schur_HIP (slampp_hip_schur_marginal_blocks): cameras and landmarks in any mix -- two cameras that share
        no landmark, two landmarks, a camera and a landmark it does not observe; each block is summed from the dense inverse of
        the reduced camera system S, or from forward substitutions on S's sparse factor over the paths of the cameras behind
        the two columns.  ``reuse_factor``: what the previous Marginals_Pattern / Marginal_Columns / Marginal_Blocks call left.
        A handle whose analysis went to the sparse path answers through it."""
        pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
        rows, cols = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        vals = self._covariance_values(lam, reuse_factor, "Marginal_Blocks")
        dims = np.diff(np.asarray(lam.cumsum, dtype=np.int64))
        in_range = pr.size and pr.min() >= 0 and pr.max() < len(dims)
        sizes = dims[rows] * dims[cols] if in_range else np.zeros(0, dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        flat = np.empty(max(int(off[-1]), 1), dtype=np.float64)
        if not self._check(getattr(self._lib, self._covariance_entries[2])(self._h, _ptr(vals) if vals is not None else None,
                                                                          int(rows.size), _ptr(rows), _ptr(cols), _ptr(flat))):
            raise ArithmeticError("Marginal_Blocks: the system is not positive definite")
        return [flat[off[k]:off[k + 1]].reshape(int(dims[cols[k]]), int(dims[rows[k]])).T.copy() for k in range(rows.size)]

    def Joint_Marginal(self, lam, bcols, reuse_factor: bool = False) -> np.ndarray:
        """The joint marginal covariance of the block columns ``bcols`` (distinct, at least one): the dense symmetric k x k
        matrix of Lambda^-1 at every pair of them, k = the sum of their dimensions, in the listed order (GTSAM's
        jointMarginalCovariance).  The upper pairs are computed (Marginal_Blocks: in Schur mode the columns may be
        cameras and landmarks in any mix) and mirrored."""
        cols = [int(c) for c in np.atleast_1d(np.asarray(bcols, dtype=np.int64))]
        if not cols or len(set(cols)) != len(cols):
            raise ValueError("Joint_Marginal: an empty set of block columns, or one listed twice")
        pairs = [(cols[a], cols[b]) for b in range(len(cols)) for a in range(b + 1)]
        blocks = self.Marginal_Blocks(lam, pairs, reuse_factor)
        dims = np.diff(np.asarray(lam.cumsum, dtype=np.int64))
        off = np.concatenate([[0], np.cumsum(dims[cols])]).astype(np.int64)
        joint = np.empty((int(off[-1]), int(off[-1])), dtype=np.float64)
        for (a, b), blk in zip(((a, b) for b in range(len(cols)) for a in range(b + 1)), blocks):
            joint[off[a]:off[a + 1], off[b]:off[b + 1]] = blk
        return np.triu(joint) + np.triu(joint, 1).T   # (the lower triangle is never filled: symmetric bit for bit)


class CLinearSolver_HIP(_SolverBase):
    """Sparse block Cholesky on the GPU; stands where CLinearSolver_CholMod / _CSparse / _UberBlock do."""

    _Tag = "CBlockwiseLinearSolverTag"   # LinearSolverTags.h:54
    _mode = MODE_SPARSE
    _covariance_entries = ("slampp_hip_marginals_pattern", "slampp_hip_marginal_columns", "slampp_hip_marginal_blocks")

    def Marginals_Pattern(self, lam) -> np.ndarray:
        """Lambda^-1 at every stored block of Lambda (see _SolverBase._marginals_pattern; no ``reuse_factor`` here: the
        sparse C entry refuses ``values = NULL``)."""
        return self._marginals_pattern(lam)


def _block_diagonal_marginals(self, lam):
    """Block diagonal of the covariance Lambda^-1 ([n, d, d]), as CMarginals::Calculate_DenseMarginals_Recurrent_FBS
    (.., mpart_Diagonal) gives the reference's nonlinear solvers (NonlinearSolver_Lambda.h:700-760): factorization and a
    sparse inverse subset on the factor's pattern (below a dense inverse of the plan's dense top, if it has one).  One block
    size (3, 6 or 7) -> an array; a mix of block sizes up to 8 (no dense top) -> a list of blocks."""
    if not self._analyzed or self._structure_key != self._key(lam):
        self.SymbolicDecomposition_Blocky(lam)
    dims = np.diff(lam.cumsum)
    vals = np.ascontiguousarray(lam.values, dtype=np.float64)
    if np.all(dims == dims[0]):
        d = int(dims[0])
        out = np.empty((len(dims), d, d), dtype=np.float64)
        if not self._check(self._lib.slampp_hip_marginals(self._h, _ptr(vals), _ptr(out))):
            raise ArithmeticError("Marginals: the system is not positive definite")
        return out.transpose(0, 2, 1).copy()      # blocks come column-major
    # mixed block sizes: a list of d_c x d_c blocks
    flat = np.empty(int((dims.astype(np.int64) ** 2).sum()), dtype=np.float64)
    if not self._check(self._lib.slampp_hip_marginals(self._h, _ptr(vals), _ptr(flat))):
        raise ArithmeticError("Marginals: the system is not positive definite")
    off = np.concatenate([[0], np.cumsum(dims.astype(np.int64) ** 2)])
    return [flat[off[c]:off[c + 1]].reshape(int(dims[c]), int(dims[c])).T.copy() for c in range(len(dims))]


CLinearSolver_HIP.Marginals = _block_diagonal_marginals


class CLinearSolver_Schur_HIP(_SolverBase):
    """Schur-complement solver for BA systems; same public surface as CLinearSolver_Schur
    (LinearSolver_Schur.h:1472-1553, 1623).  The guided ordering (cameras = wide block columns first,
    landmarks last; LinearSolver_Schur.cpp:771-838) is computed here from the block widths."""

    _Tag = "CBlockwiseLinearSolverTag"
    _mode = MODE_SCHUR

    def __init__(self, base_solver=None, device: int = 0, devices=None, **options):
        # the reference's constructor takes (and ignores) a base solver instance
        # (LinearSolver_Schur.h:1472-1474); accepted for signature parity
        super().__init__(device=device, devices=devices, **options)
        self._cut_override = None

    def _n_matrix_cut(self, lam) -> int:
        if self._cut_override is not None:
            return int(self._cut_override)
        if getattr(lam, "n_matrix_cut", 0):
            return int(lam.n_matrix_cut)
        dims = np.diff(lam.cumsum)
        wide = dims == dims.max()
        n_cut = int(np.count_nonzero(wide))
        if n_cut == 0 or n_cut == len(dims) or not np.all(wide[:n_cut]):
            # no landmark part (the reference hands such a system to its base solver, LinearSolver_Schur.h:1635-1638), or
            # cameras and landmarks interleaved (the C++ header permutes them; this mirror does not): cut 0 sends the
            # whole of Lambda through the sparse block path, which gives the same solution
            return 0
        return n_cut

    def SymbolicDecomposition_Blocky(self, lam, b_force_guided_ordering: bool = False) -> bool:
        return super().SymbolicDecomposition_Blocky(lam)

    def Set_Changed_Landmarks(self, landmark_indices) -> None:
        """The next Solve_PosDef_Blocky updates the reduced camera system of the previous one instead of rebuilding it
        (option ``schur_incremental=1``; the reference's dog-leg solver does this from Omega = delta Lambda,
        NonlinearSolver_Lambda_DL.h:2301-): ``landmark_indices`` = the landmarks (0-based among the landmark block
        columns) whose blocks changed since the previous call; camera blocks and eta may change freely."""
        idx = np.unique(np.asarray(landmark_indices, dtype=np.int64))
        self._check(self._lib.slampp_hip_schur_set_changed_points(self._h, _ptr(idx) if idx.size else None, int(idx.size)))

    def Solve_PosDef_Blocky_MarginalPoses(self, lam, eta: np.ndarray) -> bool:
        """LinearSolver_Schur.h:1956-2143: only the landmarks are solved for (dl = C^-1 eta_l), the pose part of
        ``eta`` is zeroed."""
        if eta.dtype != np.float64 or not eta.flags.c_contiguous or eta.shape != (lam.n_scalars,):
            raise ValueError("eta must be a contiguous float64 vector of the system's dimension")
        if not self._analyzed or self._structure_key != self._key(lam):
            self.SymbolicDecomposition_Blocky(lam, True)
        vals = np.ascontiguousarray(lam.values, dtype=np.float64)
        return self._check(self._lib.slampp_hip_solve_marginal_poses(self._h, _ptr(vals), _ptr(eta)))

    def Schur_Marginals(self, lam, b_do_cam_marginals: bool = True):
        """Block diagonal of the covariance Lambda^-1, as CSchurComplement_Marginals::Schur_Marginals returns it
        (BAMarginals.h:579-806): (camera blocks [nc, dc, dc] or None, landmark blocks [np, dp, dp]); the reduced
        camera system is assembled, factored and inverted on the device.  Raises if Lambda is not positive definite."""
        if not self._analyzed or self._structure_key != self._key(lam):
            self.SymbolicDecomposition_Blocky(lam, True)
        nc = self._n_matrix_cut(lam)
        dims = np.diff(lam.cumsum)
        dc, dp = int(dims[0]), int(dims[nc])
        cams = np.empty((nc, dc, dc), dtype=np.float64) if b_do_cam_marginals else None
        pts = np.empty((len(dims) - nc, dp, dp), dtype=np.float64)
        vals = np.ascontiguousarray(lam.values, dtype=np.float64)
        ok = self._check(self._lib.slampp_hip_schur_marginals(self._h, _ptr(vals), _ptr(cams) if cams is not None else None,
                                                              _ptr(pts)))
        if not ok:
            raise ArithmeticError("Schur_Marginals: the system is not positive definite")
        # blocks are column-major and symmetric: the C-order view is the same matrix
        return cams, pts

    def schur_marginals_device_async(self, values_ptr: int, cam_cov_ptr: int, point_cov_ptr: int) -> None:
        self._check(self._lib.slampp_hip_schur_marginals_device_async(self._h, values_ptr, cam_cov_ptr or None,
                                                                      point_cov_ptr or None))

    _covariance_entries = ("slampp_hip_schur_marginals_pattern", "slampp_hip_schur_marginal_columns",
                           "slampp_hip_schur_marginal_blocks")
    Marginals_Pattern = _SolverBase._marginals_pattern


class CLambdaAssembly_HIP:
    """Lambda and eta assembled on the device from per-edge Jacobians, written where the solver reads them.

    Stands where the reference computes every edge's Hessian blocks on the host and sums them with its
    reduction plan (BaseTypes_Binary.h:759-840, NonlinearSolver_Lambda_Base.h:1634-1688), for one homogeneous
    set of binary edges.  ``lam`` supplies the block structure (it must hold block (min, max) of every edge)."""

    def __init__(self, solver: _SolverBase, lam, v0: np.ndarray, v1: np.ndarray, n_residual_dim: int):
        self._solver = solver          # keeps the solver (and its stream) alive
        self._lib = solver._lib
        self._a = C.c_void_p()
        if not solver._analyzed or solver._structure_key != solver._key(lam):
            solver.SymbolicDecomposition_Blocky(lam)
        v0 = np.ascontiguousarray(v0, dtype=np.int64)
        v1 = np.ascontiguousarray(v1, dtype=np.int64)
        if v0.shape != v1.shape or v0.ndim != 1:
            raise ValueError("v0 and v1 must be vectors of one length")
        solver._check(self._lib.slampp_hip_assembly_create(solver._h, C.byref(self._a), v0.shape[0], _ptr(v0), _ptr(v1),
                                                           int(n_residual_dim)))

    def __del__(self):
        try:
            if getattr(self, "_a", None):
                self._lib.slampp_hip_assembly_destroy(self._a)
                self._a = None
        except Exception:
            pass

    def info(self) -> dict:
        """What the handle built, by the kernel that takes it (slampp_hip_assembly_get_info): ``rd``, ``d0``, ``d1``,
        ``n_groups``, ``n_grp_cap_edges``, ``n_grp_pkg_stride``, ``n_long``, ``n_long_dim``, ``n_small``, ``n_small_elems``,
        ``n_plain_diag``, ``n_offdiag``, ``n_off_elems``, ``b_offdiag_packed``."""
        t = AssemblyInfo()
        self._solver._check(self._lib.slampp_hip_assembly_get_info(self._a, C.byref(t)))
        return {n: int(getattr(t, n)) for n, _ in AssemblyInfo._fields_ if n != "n_pad"}

    def Refresh_Lambda_device(self, J0_ptr: int, J1_ptr: int, sigma_inv_ptr: int, error_ptr: int, weight_ptr: int,
                              values_ptr: int, eta_ptr: int, unary_vertex: int = 0, unary_factor=None,
                              unary_error=None, accumulate: bool = False) -> None:
        """Enqueues the assembly on the solver's stream (device pointers as integers; ``weight_ptr`` 0 = no
        robust weights).  ``unary_factor`` is the d x d factor U of the anchor (column-major) and
        ``unary_error`` its error vector, both host arrays or None."""
        uf = None if unary_factor is None else np.ascontiguousarray(unary_factor, dtype=np.float64)
        ue = None if unary_error is None else np.ascontiguousarray(unary_error, dtype=np.float64)
        self._solver._check(self._lib.slampp_hip_assemble_device_async(
            self._a, J0_ptr, J1_ptr, sigma_inv_ptr, error_ptr, weight_ptr or None, int(unary_vertex),
            None if uf is None else _ptr(uf), None if ue is None else _ptr(ue), values_ptr, eta_ptr, int(bool(accumulate))))

    def Linearize_device(self, edge_type: int, state_ptr: int, measurement_ptr: int, J0_ptr: int, J1_ptr: int, error_ptr: int,
                         params_ptr: int = 0) -> None:
        """Every edge's error and Jacobians from the vertex states, written where Refresh_Lambda_device reads them
        (slampp_hip_linearize_device_async; the reference's Calculate_Jacobians_Expectation_Error).  ``edge_type``: EDGE_SE2,
        EDGE_SE3, EDGE_P2C_XYZ, EDGE_POSE_LANDMARK_2D, EDGE_POSE_LANDMARK_3D or EDGE_P2SC_XYZ, matching this edge set's
        dimensions; ``state_ptr``: the states in the layout of eta; ``params_ptr``: per block column five intrinsics
        (EDGE_P2C_XYZ) or six, the baseline last (EDGE_P2SC_XYZ); 0 for the other types.  Enqueue-only."""
        self._solver._check(self._lib.slampp_hip_linearize_device_async(
            self._a, int(edge_type), state_ptr or None, measurement_ptr or None, params_ptr or None, J0_ptr or None, J1_ptr or None,
            error_ptr or None))

    def Chi2_device(self, sigma_inv_ptr: int, error_ptr: int, weight_ptr: int, out_ptr: int) -> None:
        """*out = sum over the edges of w err^T Sigma^-1 err in a fixed order (slampp_hip_chi_squared_device_async);
        ``weight_ptr`` 0 = no robust weights.  Enqueue-only."""
        self._solver._check(self._lib.slampp_hip_chi_squared_device_async(self._a, sigma_inv_ptr or None, error_ptr or None,
                                                                          weight_ptr or None, out_ptr or None))

    def Set_Robust(self, kernel, basis: int = ROBUST_BASIS_ERROR_NORM, mode: int = ROBUST_MODE_REFERENCE, scale: float = 1.0,
                   param: float = None) -> None:
        """A robust kernel for this edge set (slampp_hip_assembly_set_robust): ``kernel`` ROBUST_HUBER, _CAUCHY, _TUKEY or
        _WELSCH, w(s) of the reference's loss functions with a = ``param`` (None: the reference's default); ``basis`` what s is
        -- ROBUST_BASIS_ERROR_NORM |err| / scale, _CHI2 err^T Sigma^-1 err / scale, _MAHALANOBIS sqrt(err^T Sigma^-1 err) /
        scale; ``mode`` how the LM loop applies the weight -- ROBUST_MODE_REFERENCE as the reference's robust edges do, or
        ROBUST_MODE_LOSS (MAHALANOBIS only), which minimises sum 2 scale^2 rho(s).  The reference's CEdgePose3D is
        ``Set_Robust(ROBUST_HUBER, ROBUST_BASIS_ERROR_NORM, ROBUST_MODE_REFERENCE, 0.3, 1.345)``.  The handle then owns an
        array of a weight per edge; ``Set_Robust(None)`` frees it and takes the kernel off."""
        if kernel is None:
            self._solver._check(self._lib.slampp_hip_assembly_set_robust(self._a, None))
            return
        spec = Robust(int(kernel), int(basis), int(mode), float(scale),
                      float(ROBUST_DEFAULT_PARAM.get(int(kernel), 0.0) if param is None else param))
        self._solver._check(self._lib.slampp_hip_assembly_set_robust(self._a, C.byref(spec)))

    def Robust_Weights_ptr(self) -> int:
        """The device pointer of the handle's weight array, 0 where no robust kernel is set (slampp_hip_assembly_robust_weights)."""
        p = C.c_void_p()
        self._solver._check(self._lib.slampp_hip_assembly_robust_weights(self._a, C.byref(p)))
        return p.value or 0

    def Robust_Weights_device(self, sigma_inv_ptr: int, error_ptr: int, weight_out_ptr: int = 0) -> None:
        """w(s) of every edge into ``weight_out_ptr`` (0: the handle's array) from the errors Linearize_device wrote
        (slampp_hip_robust_weights_device_async); ``sigma_inv_ptr`` may be 0 with ROBUST_BASIS_ERROR_NORM.  Enqueue-only."""
        self._solver._check(self._lib.slampp_hip_robust_weights_device_async(self._a, sigma_inv_ptr or None, error_ptr or None,
                                                                             weight_out_ptr or None))

    def Robust_Scale_device(self, J0_ptr: int, J1_ptr: int, error_ptr: int, weight_ptr: int = 0) -> None:
        """J0, J1 and the errors of every edge times sqrt(w) of the edge, in place (slampp_hip_robust_scale_device_async);
        ``weight_ptr`` 0: the handle's array.  Enqueue-only."""
        self._solver._check(self._lib.slampp_hip_robust_scale_device_async(self._a, weight_ptr or None, J0_ptr or None, J1_ptr or None,
                                                                           error_ptr or None))

    def Robust_Chi2_device(self, sigma_inv_ptr: int, error_ptr: int, out_ptr: int) -> None:
        """*out = sum over the edges of 2 scale^2 rho(s) in a fixed order (slampp_hip_robust_chi_squared_device_async;
        ROBUST_BASIS_MAHALANOBIS only).  Enqueue-only."""
        self._solver._check(self._lib.slampp_hip_robust_chi_squared_device_async(self._a, sigma_inv_ptr or None, error_ptr or None,
                                                                                 out_ptr or None))


def Refresh_Lambda_sets_device(assemblies, pointer_sets, values_ptr: int, eta_ptr: int, unary_vertex: int = 0, unary_factor=None,
                               unary_error=None, accumulate: bool = False) -> None:
    """Every edge type of one Lambda in one call (slampp_hip_assemble_sets_device_async): ``assemblies`` a list of
    CLambdaAssembly_HIP of the same solver, ``pointer_sets`` their (J0, J1, sigma_inv, error, weight) device pointers."""
    sets = (EdgeSetPtrs * len(assemblies))()
    for i, (a, ptrs) in enumerate(zip(assemblies, pointer_sets)):
        sets[i].p_assembly = a._a
        sets[i].p_J0_dev, sets[i].p_J1_dev, sets[i].p_sigma_inv_dev, sets[i].p_error_dev = [int(p) for p in ptrs[:4]]
        sets[i].p_weight_dev = int(ptrs[4]) if len(ptrs) > 4 and ptrs[4] else None
    uf = None if unary_factor is None else np.ascontiguousarray(unary_factor, dtype=np.float64)
    ue = None if unary_error is None else np.ascontiguousarray(unary_error, dtype=np.float64)
    solver = assemblies[0]._solver
    solver._check(solver._lib.slampp_hip_assemble_sets_device_async(
        sets, len(assemblies), int(unary_vertex), None if uf is None else _ptr(uf), None if ue is None else _ptr(ue),
        values_ptr, eta_ptr, int(bool(accumulate))))


_EDGE_DIMS = {EDGE_SE2: (3, 3, 3, 3), EDGE_SE3: (6, 6, 6, 6), EDGE_P2C_XYZ: (6, 3, 2, 2),       # d0, d1, rd, measurement
              EDGE_POSE_LANDMARK_2D: (3, 2, 2, 2), EDGE_POSE_LANDMARK_3D: (6, 3, 3, 3), EDGE_P2SC_XYZ: (6, 3, 3, 3)}


class CLevenbergMarquardt_HIP:
    """The reference's ``CNonlinearSolver_Lambda_LM`` with ``CLevenbergMarquardt_Baseline`` (NonlinearSolver_Lambda_LM.h:151-223,
    915-1115) decided on the device: ``Begin`` initialises the scalars, ``Iterate(n)`` enqueues n rounds of linearize ->
    assemble -> damp -> factor_solve -> gain -> plus -> errors -> chi^2 -> decide -> commit, and nothing is waited for until
    ``Sync`` (slampp_hip_lm_begin_device_async, slampp_hip_lm_iterate_device_async).

    ``edge_sets``: a list of dicts with ``assembly`` (a CLambdaAssembly_HIP of ``solver``), ``edge_type`` (EDGE_*),
    ``measurement`` [E, 3 | 6 | 2 | 2 | 3 | 3], ``sigma_inv`` [E, rd, rd] (every matrix column-major, as the assembly reads
    them), and optionally ``params`` (per block column five intrinsics for EDGE_P2C_XYZ, six with the baseline for
    EDGE_P2SC_XYZ) and ``weight`` [E]; arrays or CUDA tensors.  A set
    may carry ``robust`` instead of ``weight``: a dict of the arguments of ``CLambdaAssembly_HIP.Set_Robust`` (``kernel``,
    ``basis``, ``mode``, ``scale``, ``param``), which is set on the set's assembly; the loop then computes the weights itself.
    ``lam``: Lambda's block structure, as CLambdaAssembly_HIP takes it.
    ``vertex_ranges``: (VERTEX_*, first, last) triples covering every block column once.  ``unary``: (vertex, factor, error)
    with host arrays (error may be None), or None.  The object owns the state (``self.state``, a CUDA tensor of n_scalars
    doubles, a copy of ``state``) and every scratch array; memory comes from torch."""

    def __init__(self, solver: _SolverBase, lam, edge_sets, vertex_ranges, state, unary=None, trace_capacity: int = 256):
        import torch
        self._torch, self._solver, self._lib = torch, solver, solver._lib
        if not solver._analyzed or solver._structure_key != solver._key(lam):
            solver.SymbolicDecomposition_Blocky(lam)
        stats = Stats()
        solver._check(self._lib.slampp_hip_get_stats(solver._h, C.byref(stats)))
        n = int(stats.n_scalars)
        dev = torch.device("cuda", solver._device)

        def tensor(a):
            if a is None:
                return None
            if isinstance(a, torch.Tensor):
                return a.to(device=dev, dtype=torch.float64).contiguous()
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)

        def scratch(k):
            return torch.zeros(max(int(k), 1), dtype=torch.float64, device=dev)

        def ptr(t):
            return None if t is None else t.data_ptr()
        self.state = tensor(state).clone()
        if self.state.numel() != n:
            raise ValueError("state must hold n_scalars doubles")
        self._keep = []                                   # the tensors and handles the problem points at
        self._sets = (LmEdgeSet * max(len(edge_sets), 1))()
        for i, s in enumerate(edge_sets[:LM_MAX_SETS]):
            d0, d1, rd, md = _EDGE_DIMS.get(int(s["edge_type"]), (8, 8, 8, 8))
            z, sigma = tensor(s["measurement"]), tensor(s["sigma_inv"])
            e = z.numel() // md
            params, weight = tensor(s.get("params")), tensor(s.get("weight"))
            if s.get("robust") is not None:
                if weight is not None:
                    raise ValueError("an edge set takes robust or weight, not both")
                s["assembly"].Set_Robust(**s["robust"])
            J0, J1, err = scratch(e * rd * d0), scratch(e * rd * d1), scratch(e * rd)
            self._keep += [s["assembly"], z, sigma, params, weight, J0, J1, err]
            t = self._sets[i]
            t.p_assembly, t.n_edge_type = s["assembly"]._a, int(s["edge_type"])
            t.p_measurement_dev, t.p_params_dev, t.p_sigma_inv_dev, t.p_weight_dev = ptr(z), ptr(params), ptr(sigma), ptr(weight)
            t.p_J0_dev, t.p_J1_dev, t.p_error_dev = ptr(J0), ptr(J1), ptr(err)
        self._ranges = (LmVertexRange * max(len(vertex_ranges), 1))()
        for i, (kind, first, last) in enumerate(vertex_ranges):
            self._ranges[i].n_vertex_type, self._ranges[i].n_first_vertex, self._ranges[i].n_last_vertex = int(kind), int(first), int(last)
        self.trial, self.eta, self.dx = scratch(n), scratch(n), scratch(n)
        self.values = scratch(lam.values.shape[0])
        self.scalars_dev, self.chi_parts = scratch(LM_SCALARS), scratch(LM_MAX_SETS)
        self.trace_capacity = int(trace_capacity)
        self.trace_dev = scratch(self.trace_capacity * LM_TRACE_RECORD)
        p = self._problem = LmProblem()
        p.p_solver = solver._h
        p.n_sets, p.p_sets = len(edge_sets), self._sets
        p.n_ranges, p.p_ranges = len(vertex_ranges), self._ranges
        p.n_unary_vertex = -1
        if unary is not None:
            vertex, factor, error = unary
            self._unary = (np.ascontiguousarray(factor, dtype=np.float64),
                           None if error is None else np.ascontiguousarray(error, dtype=np.float64))
            p.n_unary_vertex, p.p_unary_factor = int(vertex), self._unary[0].ctypes.data
            p.p_unary_error = None if error is None else self._unary[1].ctypes.data
        p.p_state_dev, p.p_trial_dev, p.p_values_dev = self.state.data_ptr(), self.trial.data_ptr(), self.values.data_ptr()
        p.p_eta_dev, p.p_dx_dev, p.p_lm_dev = self.eta.data_ptr(), self.dx.data_ptr(), self.scalars_dev.data_ptr()
        p.p_chi_parts_dev, p.p_trace_dev, p.n_trace_capacity = self.chi_parts.data_ptr(), self.trace_dev.data_ptr(), self.trace_capacity
        torch.cuda.synchronize(dev)                       # (torch filled the arrays on its own stream)

    def Begin(self, f_alpha: float = 0.0, f_tau: float = 1e-3, f_min_dx_norm: float = 0.0, n_max_iterations: int = 1 << 30,
              n_extra_on_reject: int = 10) -> None:
        """The scalars of a new loop from ``self.state``: alpha = f_tau max diag of the edges' Hessians where f_tau > 0,
        else f_alpha; nu = 2; chi^2 of the state.  Enqueue-only."""
        self._solver._check(self._lib.slampp_hip_lm_begin_device_async(
            C.byref(self._problem), float(f_alpha), float(f_tau), float(f_min_dx_norm), int(n_max_iterations), int(n_extra_on_reject)))

    def Iterate(self, n_rounds: int) -> None:
        """Enqueues n_rounds rounds; those after the status left 0 change nothing the caller can see.  Enqueue-only."""
        self._solver._check(self._lib.slampp_hip_lm_iterate_device_async(C.byref(self._problem), int(n_rounds)))

    def Sync(self):
        """Waits once (slampp_hip_sync) and returns (positive definite, scalars [LM_SCALARS], trace [records, LM_TRACE_RECORD])
        as numpy arrays; False is slampp_hip_sync's SLAMPP_HIP_NOT_POSDEF, and the scalars' status says the same."""
        ok = self._solver.sync()
        scalars = self.scalars_dev.cpu().numpy().copy()
        n = min(int(scalars[LM_N_RECORDS]), self.trace_capacity)
        trace = self.trace_dev[:n * LM_TRACE_RECORD].cpu().numpy().reshape(n, LM_TRACE_RECORD).copy()
        return ok, scalars, trace

    def Optimize(self, n_max_iterations: int = 5, f_min_dx_norm: float = 0.01, f_tau: float = 1e-3, f_alpha: float = 0.0,
                 n_extra_on_reject: int = 10):
        """CNonlinearSolver_Lambda_LM::Optimize(n_max_iteration_num, f_min_dx_norm): every round it can take is enqueued at
        once, then one wait.  Returns what ``Sync`` returns."""
        self.Begin(f_alpha, f_tau, f_min_dx_norm, n_max_iterations, n_extra_on_reject)
        if n_max_iterations > 0:
            self.Iterate(n_max_iterations + max(int(n_extra_on_reject), 0))
        return self.Sync()
