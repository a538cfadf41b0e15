"""The block-sparse solve as a differentiable PyTorch operation, in both modes.

``solve(solver, lam, values, eta)`` returns ``x = M(values)^-1 eta`` as a tensor that carries a ``backward``; ``M(v)`` is the
symmetric matrix slampp_hip_multiply defines from the packed values ``v`` of the block structure of ``lam``: a stored upper
block (r, c), r < c, stands at (r, c) and transposed at (c, r), diagonal blocks are the full d x d blocks.  With an upstream
gradient ``x_bar``::

    g        = M^-1 x_bar                       one more right-hand side on the KEPT factor
    eta_bar  = g
    v_bar(r, c) = -(g_r x_c^T + x_r g_c^T)      every stored block r < c
    v_bar(r, r) = - g_r x_r^T                   every diagonal block

so a backward pass costs two substitutions (slampp_hip_solve_again_device_async) and one streaming kernel
(slampp_hip_pattern_outer_device_async, launched only when ``values`` needs a gradient); there is no second factorization.
The function is once differentiable.

Calling rules.  ``solver`` is a CLinearSolver_HIP or a CLinearSolver_Schur_HIP; ``lam`` supplies the block structure only:
it is analyzed on first use and again when its structure key changes, as Solve_PosDef_Blocky decides.  ``values``
(``lam.values.shape``) and ``eta`` (``(lam.n_scalars,)``) are contiguous float64 CUDA tensors on the solver's device;
anything else raises TypeError / ValueError before the library is called.  The forward pass waits for the device once
(slampp_hip_sync: that is how a matrix that is not positive definite is reported -- torch.linalg.LinAlgError, and nothing is
saved for backward); the backward pass only enqueues.

Who owns the factor.  A handle keeps ONE factor.  Every forward pass remembers the solver object's factor generation
(``solver.factor_generation``), which counts up with every call through the Python wrapper that factors, drops the factor
or changes the structure: another ``solve``, Solve_PosDef*, factor_solve_device*, a batch, the covariance calls,
Free_Memory, a new structure (also through Multiply / Pattern_Outer on another system).  If the generation has moved by the
time of the backward pass, the factor is someone else's and backward calls slampp_hip_factor_solve_device_async on the
saved values and ``x_bar`` instead (after analyzing its own structure again, if the handle has been given another): the same
``M^-1 x_bar``, at the price of a factorization.  A Schur-mode solver without the option ``schur_keep=1`` (or
``schur_incremental``) keeps no factor a re-solve could use, and takes that route every time; it never raises for this
reason.  ``solver.n_backward_refactorizations`` counts these events.  Calls that reach the handle around the Python
wrapper (the C ABI directly) are not seen.

Streams.  The library enqueues on its own stream, wrapped once per solver as ``torch.cuda.ExternalStream``.  Before a
call enqueues, that stream waits for torch's current stream; afterwards torch's current stream waits for it.  So the
inputs are ready when the library reads them, the outputs are ready for whatever torch enqueues next, and no tensor handed
to the library is freed and reused ahead of the work that reads it.  There is no torch.cuda.synchronize().

``solve_batch(solver, lam, values[K, n_values], eta[K, n_scalars])``: K <= 64 value sets of one structure, sparse mode
only (slampp_hip_factor_solve_batch_device_async + slampp_hip_sync_batch; a member that is not positive definite raises and
is named).  A batch keeps no factors, so its backward pass is the same batched call on ``(values, x_bar)`` -- K
factorizations, the documented cost -- followed by the batched outer-product kernel.  The tensors are passed as they are
(rows contiguous, any row stride of at least a row); odd strides are solved member by member inside the library, with the
same results.

``solve_multi(solver, lam, values, eta[K, n_scalars])``: K <= 256 right-hand sides on ONE set of values, in both modes (rows
contiguous, any row stride of at least a row).  Forward: slampp_hip_factor_solve_device_async on row 0, then the rows after it
in one slampp_hip_solve_columns_device_async on the factor that left, and one wait.  Backward: ``g = M^-1 x_bar`` for all rows in
one slampp_hip_solve_columns_device_async on the kept factor -- under the generation rule above --, ``eta_bar = g`` and
``v_bar = -sum_k P(g_k, x_k)`` in one launch (slampp_hip_pattern_outer_sum_device_async).  If the factor is someone else's by
then, row 0 of ``g`` factors the saved values again and the other rows follow on that factor: one factorization.  A
Schur-mode solver without ``schur_keep=1`` (or ``schur_incremental``) keeps no factor: it solves row by row with
slampp_hip_factor_solve_device_async, forward and backward (K factorizations each), and never raises for it.
``solver.n_backward_refactorizations`` counts the factorizations backward passes had to make: 1, or K for such a solver.

``logdet(solver, lam, values)`` returns ``log det M(values)`` as a 0-dim float64 tensor on the solver's device, once
differentiable in ``values`` (both modes).  Forward: slampp_hip_logdet_device_async with ``b_reuse_factor = 0`` -- the values are
factored and twice the sum of log of the factor's pivots is taken on the device, Schur mode adding every landmark's
``log det C_p`` --, then one wait (a matrix that is not positive definite raises torch.linalg.LinAlgError).  Backward:
``v_bar = y_bar * w * Sigma`` with ``Sigma = M^-1`` on the structure's pattern from the pattern-covariance device call of the
solver's mode on the saved values, and ``w`` = 2 on off-diagonal blocks (a stored block (r, c), r < c, stands at (r, c) and
transposed at (c, r)), 1 on diagonal blocks (whose gradient is Sigma(r, r)^T = Sigma(r, r)); ``w`` is cached on the solver
as a device tensor per structure key.  The covariance call factors the saved values AGAIN: a backward pass costs one
factorization plus the covariance recursion, and it leaves the handle's factor as that call leaves it.  Where the covariance
call is unsupported (sparse mode: block columns wider than 8), backward raises a RuntimeError naming the limit; the forward
pass works regardless.

``quad_form(solver, lam, values, B[k, n_scalars])`` returns ``G = B M^-1 B^T`` (k x k, k <= 48), differentiable in ``values`` and
``B``; sparse mode with block columns of at most 8 (the library refuses anything else: NotImplementedError in Schur mode).
Forward: the values are factored as ``solve`` factors them (slampp_hip_factor_solve_device_async on a zero vector, which
leaves the kept factor), ``Y = L^-1 P B^T`` by the forward half alone (slampp_hip_solve_half_columns_device_async) on a copy
of B, ``G = Y^T Y`` by slampp_hip_gram_device_async -- bitwise symmetric --, and ``X = P^T L^-T Y = M^-1 B^T`` by the backward
half on a copy of Y, saved for backward (skipped where neither input requires a gradient); one wait.  Backward, with an
upstream ``G_bar``: ``B_bar = (G_bar + G_bar^T) X`` and ``v_bar = -sum_a P(x_a, w_a)`` with ``W = G_bar X`` in one slampp_hip_pattern_outer_sum_device_async, because
``dG_ab = -x_a^T dM x_b = -<dv, P(x_a, x_b)>``.  Everything backward needs is in X: it reads no factor, so it does not matter
whose factor the handle holds by then, and nothing is factored again; a handle that has been given another structure since
is given this one again (analyzed, as the other backward passes do), because the outer products run on the handle's structure.

``sample(solver, lam, values, Z[k, n_scalars])`` returns rows ``x = P^T L^-T z`` (the backward half alone): for standard
normal z, samples of covariance ``M^-1``.  ``whiten(solver, lam, values, B[k, n_scalars])`` returns rows ``L^-1 P b`` (the
forward half alone; their squared norms are ``b^T M^-1 b``) and the block permutation P (``factor_structure()["perm"]``: new
block j is the caller's block perm[j]).  Neither is differentiable: the derivative of the Cholesky factor is not built
here.  Both return detached tensors and raise if ``values`` requires a gradient; k <= 256.

``dense_from_packed`` and ``pattern_outer_reference`` restate M(v) and the outer product in plain torch / numpy: the
yardsticks of the tests.
"""
from __future__ import annotations

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .hip_solver import CLinearSolver_HIP, CLinearSolver_Schur_HIP, MODE_SPARSE, HALF_FORWARD, HALF_BACKWARD, GRAM_MAX_COLUMNS

MAX_BATCH = 64     # SLAMPP_HIP_MAX_BATCH
MAX_COLUMNS = 256  # SLAMPP_HIP_SOLVE_MAX_COLUMNS


# ---- the yardsticks ----

def _element_rows_cols(lam):
    """(row, col, offdiag) of every packed value of ``lam``'s structure: its scalar row and column in the full matrix (blocks in
    block-CSC order, each column-major) and whether its block lies off the diagonal."""
    cs = np.asarray(lam.cumsum, dtype=np.int64)
    dims = np.diff(cs)
    brow = np.asarray(lam.brow_idx, dtype=np.int64)
    bcol = np.repeat(np.arange(len(dims), dtype=np.int64), np.diff(lam.bcol_ptr))
    sizes = dims[brow] * dims[bcol]
    off = np.concatenate([[0], np.cumsum(sizes)])
    blk = np.repeat(np.arange(len(brow), dtype=np.int64), sizes)
    local = np.arange(int(off[-1]), dtype=np.int64) - off[blk]
    d_r = dims[brow][blk]
    return cs[brow][blk] + local % d_r, cs[bcol][blk] + local // d_r, (brow != bcol)[blk]


def dense_from_packed(lam, values: torch.Tensor) -> torch.Tensor:
    """The dense symmetric M(values) of ``lam``'s structure, as a differentiable function of ``values`` (a scatter)."""
    row, col, offdiag = _element_rows_cols(lam)
    n = int(lam.cumsum[-1])
    src = np.arange(row.shape[0], dtype=np.int64)
    idx = np.concatenate([row * n + col, (col * n + row)[offdiag]])
    src = np.concatenate([src, src[offdiag]])
    flat = values.new_zeros(n * n).index_put((torch.from_numpy(idx).to(values.device),),
                                             values[torch.from_numpy(src).to(values.device)])
    return flat.reshape(n, n)


def pattern_outer_reference(lam, a: np.ndarray, b: np.ndarray, alpha: float = 1.0) -> np.ndarray:
    """alpha P(a, b) on ``lam``'s pattern in numpy: alpha (a_r b_c^T + b_r a_c^T) at the stored blocks r < c, alpha a_r b_r^T
    at the diagonal blocks; shaped like ``lam.values``."""
    row, col, offdiag = _element_rows_cols(lam)
    out = a[row] * b[col]
    out[offdiag] += (b[row] * a[col])[offdiag]
    return alpha * out


# ---- the library's stream beside torch's ----

def _solver_stream(solver) -> torch.cuda.Stream:
    stream = getattr(solver, "_torch_stream", None)
    if stream is None:
        stream = solver._torch_stream = torch.cuda.ExternalStream(solver.stream(), device=torch.device("cuda", solver._device))
    return stream


def _enqueue(solver, fn) -> None:
    """fn() enqueues on the solver's stream, behind what torch's current stream holds and ahead of what it gets next."""
    ours, theirs = _solver_stream(solver), torch.cuda.current_stream(torch.device("cuda", solver._device))
    ours.wait_stream(theirs)
    try:
        fn()
    finally:                                    # (also where fn() raised after it had enqueued something)
        theirs.wait_stream(ours)


# ---- checks (before any call into the library) ----

def _check_tensor(solver, t, name: str, shape) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.dtype != torch.float64:
        raise TypeError(f"{name} must be float64, not {t.dtype}")
    if t.device.type != "cuda" or t.device.index != solver._device:
        raise ValueError(f"{name} must live on the solver's device cuda:{solver._device}, not on {t.device}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have the shape {tuple(shape)}, not {tuple(t.shape)}")
    if t.stride(-1) != 1 and t.shape[-1] > 1:
        raise ValueError(f"{name} must be contiguous")


def _check_solver(solver) -> None:
    if not isinstance(solver, (CLinearSolver_HIP, CLinearSolver_Schur_HIP)):
        raise TypeError("solver must be a CLinearSolver_HIP or a CLinearSolver_Schur_HIP")


def _require_analysis(solver, lam) -> None:
    if not solver._analyzed or solver._structure_key != solver._key(lam):
        solver.SymbolicDecomposition_Blocky(lam)


def _keeps_factor(solver) -> bool:
    """Does a solve of this solver leave a factor slampp_hip_solve_again_device_async can work from?"""
    if solver._mode == MODE_SPARSE:
        return True
    return bool(solver._options_now.get("schur_keep", 0) or solver._options_now.get("schur_incremental", 0))


# ---- one system ----

class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, eta, solver, lam):
        x = eta.clone()
        v = values.detach()
        _enqueue(solver, lambda: solver.factor_solve_device_async(v.data_ptr(), x.data_ptr()))
        if not solver.sync():
            raise torch.linalg.LinAlgError("solve: the matrix is not positive definite")
        ctx.solver, ctx.lam, ctx.generation = solver, lam, solver.factor_generation
        ctx.save_for_backward(values, x)
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, x_bar):
        values, x = ctx.saved_tensors
        solver, lam = ctx.solver, ctx.lam
        g = x_bar.clone(memory_format=torch.contiguous_format)
        v_bar = torch.empty_like(values) if ctx.needs_input_grad[0] else None
        b_kept = ctx.generation == solver.factor_generation and _keeps_factor(solver)
        if not b_kept:
            _require_analysis(solver, lam)          # (the handle may have been given another structure since)

        def work():
            if b_kept:
                solver.solve_again_device(g.data_ptr())
            else:
                solver.factor_solve_device_async(values.data_ptr(), g.data_ptr())
            if v_bar is not None:
                solver.pattern_outer_device(g.data_ptr(), x.data_ptr(), v_bar.data_ptr(), -1.0, 0.0)
        _enqueue(solver, work)
        if not b_kept:
            solver.n_backward_refactorizations += 1
            ctx.generation = solver.factor_generation     # the handle's factor is this node's again
        return v_bar, (g if ctx.needs_input_grad[1] else None), None, None


def solve(solver, lam, values: torch.Tensor, eta: torch.Tensor) -> torch.Tensor:
    """x = M(values)^-1 eta on the block structure of ``lam``, differentiable in ``values`` and ``eta`` (module docstring)."""
    _check_solver(solver)
    _check_tensor(solver, values, "values", (int(lam.values.shape[0]),))
    _check_tensor(solver, eta, "eta", (int(lam.cumsum[-1]),))
    _require_analysis(solver, lam)
    return _Solve.apply(values, eta, solver, lam)


# ---- K right-hand sides on one set of values ----

def _solve_rows(solver, values, rows, b_factor_first: bool) -> int:
    """Enqueues M(values)^-1 on every row of ``rows`` (K, n_scalars; contiguous) in place and returns the number of
    factorizations that took.  ``b_factor_first``: row 0 by slampp_hip_factor_solve_device_async, which installs the factor
    the other rows are solved from (slampp_hip_solve_columns_device_async); a Schur solver that keeps no factor solves every
    row with a factorization of its own.  Otherwise all rows from the factor in place."""
    n_rows, n_ld = rows.shape[0], rows.stride(0)
    if not b_factor_first:
        solver.solve_columns_device(rows.data_ptr(), n_ld, n_rows)
        return 0
    solver.factor_solve_device_async(values.data_ptr(), rows.data_ptr())
    if n_rows == 1:
        return 1
    if _keeps_factor(solver):
        solver.solve_columns_device(rows.data_ptr() + 8 * n_ld, n_ld, n_rows - 1)
        return 1
    for k in range(1, n_rows):
        solver.factor_solve_device_async(values.data_ptr(), rows.data_ptr() + 8 * k * n_ld)
    return n_rows


class _SolveMulti(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, eta, solver, lam):
        x = eta.clone(memory_format=torch.contiguous_format)
        v = values.detach()
        _enqueue(solver, lambda: _solve_rows(solver, v, x, True))
        if not solver.sync():
            raise torch.linalg.LinAlgError("solve_multi: the matrix is not positive definite")
        ctx.solver, ctx.lam, ctx.generation = solver, lam, solver.factor_generation
        ctx.save_for_backward(values, x)
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, x_bar):
        values, x = ctx.saved_tensors
        solver, lam = ctx.solver, ctx.lam
        g = x_bar.clone(memory_format=torch.contiguous_format)
        v_bar = torch.empty_like(values) if ctx.needs_input_grad[0] else None
        b_kept = ctx.generation == solver.factor_generation and _keeps_factor(solver)
        if not b_kept:
            _require_analysis(solver, lam)          # (the handle may have been given another structure since)
        n_factorizations = []

        def work():
            n_factorizations.append(_solve_rows(solver, values, g, not b_kept))
            if v_bar is not None:
                solver.pattern_outer_sum_device(g.shape[0], g.data_ptr(), g.stride(0), x.data_ptr(), x.stride(0),
                                                v_bar.data_ptr(), -1.0, 0.0)
        _enqueue(solver, work)
        if not b_kept:
            solver.n_backward_refactorizations += n_factorizations[0]
            ctx.generation = solver.factor_generation     # the handle's factor is this node's again
        return v_bar, (g if ctx.needs_input_grad[1] else None), None, None


def solve_multi(solver, lam, values: torch.Tensor, eta: torch.Tensor) -> torch.Tensor:
    """x[k] = M(values)^-1 eta[k] for K <= 256 right-hand sides on ONE set of values, differentiable in both (module docstring)."""
    _check_solver(solver)
    _check_tensor(solver, values, "values", (int(lam.values.shape[0]),))
    n_scalars = int(lam.cumsum[-1])
    if isinstance(eta, torch.Tensor) and (eta.dim() != 2 or not 1 <= eta.shape[0] <= MAX_COLUMNS):
        raise ValueError(f"eta must be a tensor of the shape (K, n_scalars), 1 <= K <= {MAX_COLUMNS}")
    _check_tensor(solver, eta, "eta", (eta.shape[0] if isinstance(eta, torch.Tensor) else 1, n_scalars))
    if eta.shape[0] > 1 and eta.stride(0) < n_scalars:
        raise ValueError("the rows of eta overlap (row stride below the row length)")
    _require_analysis(solver, lam)
    return _SolveMulti.apply(values, eta, solver, lam)


# ---- K value sets of one structure ----

class _SolveBatch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, eta, solver, lam):
        n_batch = values.shape[0]
        x = eta.clone()
        v = values.detach()
        _enqueue(solver, lambda: solver.factor_solve_batch_device_async(n_batch, v.data_ptr(), v.stride(0), x.data_ptr(), x.stride(0)))
        bad = [k for k, ok in enumerate(solver.sync_batch(n_batch)) if not ok]
        if bad:
            raise torch.linalg.LinAlgError(f"solve_batch: the matrices of the members {bad} are not positive definite")
        ctx.solver, ctx.lam = solver, lam
        ctx.save_for_backward(values, x)
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, x_bar):
        values, x = ctx.saved_tensors
        solver, n_batch = ctx.solver, values.shape[0]
        g = x_bar.clone(memory_format=torch.contiguous_format)
        v_bar = torch.empty((n_batch, values.shape[1]), dtype=values.dtype, device=values.device) if ctx.needs_input_grad[0] else None
        _require_analysis(solver, ctx.lam)

        def work():
            solver.factor_solve_batch_device_async(n_batch, values.data_ptr(), values.stride(0), g.data_ptr(), g.stride(0))
            if v_bar is not None:
                solver.pattern_outer_batch_device(n_batch, g.data_ptr(), g.stride(0), x.data_ptr(), x.stride(0), v_bar.data_ptr(),
                                                  v_bar.stride(0), -1.0, 0.0)
        _enqueue(solver, work)
        return v_bar, (g if ctx.needs_input_grad[1] else None), None, None


def solve_batch(solver, lam, values: torch.Tensor, eta: torch.Tensor) -> torch.Tensor:
    """x[k] = M(values[k])^-1 eta[k] for K <= 64 value sets of ``lam``'s structure (sparse mode), differentiable in both."""
    _check_solver(solver)
    if solver._mode != MODE_SPARSE:
        raise TypeError("solve_batch: sparse mode only (a CLinearSolver_HIP)")
    if not isinstance(values, torch.Tensor) or values.dim() != 2 or not 1 <= values.shape[0] <= MAX_BATCH:
        raise ValueError(f"values must be a tensor of the shape (K, n_values), 1 <= K <= {MAX_BATCH}")
    n_batch, n_values, n_scalars = values.shape[0], int(lam.values.shape[0]), int(lam.cumsum[-1])
    _check_tensor(solver, values, "values", (n_batch, n_values))
    _check_tensor(solver, eta, "eta", (n_batch, n_scalars))
    if n_batch > 1 and (values.stride(0) < n_values or eta.stride(0) < n_scalars):
        raise ValueError("the members of values / eta overlap (row stride below the row length)")
    _require_analysis(solver, lam)
    return _SolveBatch.apply(values, eta, solver, lam)


# ---- log det M(values) ----

def _logdet_weights(solver, lam, like: torch.Tensor) -> torch.Tensor:
    """w of the module docstring for ``lam``'s structure: 2 at the values of off-diagonal blocks, 1 at those of diagonal
    blocks; one device tensor per structure key, kept on the solver."""
    key = solver._key(lam)
    cached = getattr(solver, "_logdet_w", None)
    if cached is None or cached[0] != key:
        offdiag = _element_rows_cols(lam)[2]
        w = torch.from_numpy(np.where(offdiag, 2.0, 1.0)).to(like.device)
        cached = solver._logdet_w = (key, w)
    return cached[1]


class _Logdet(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, solver, lam):
        out = torch.empty((), dtype=torch.float64, device=values.device)
        v = values.detach()
        _enqueue(solver, lambda: solver.logdet_device(v.data_ptr(), out.data_ptr(), False))
        if not solver.sync():
            raise torch.linalg.LinAlgError("logdet: the matrix is not positive definite")
        ctx.solver, ctx.lam = solver, lam
        ctx.save_for_backward(values)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, y_bar):
        values, = ctx.saved_tensors
        solver, lam = ctx.solver, ctx.lam
        _require_analysis(solver, lam)              # (the handle may have been given another structure since)
        sigma = torch.empty_like(values)
        try:
            _enqueue(solver, lambda: solver.marginals_pattern_device(values.data_ptr(), sigma.data_ptr()))
        except NotImplementedError as e:
            raise RuntimeError("logdet: the gradient needs Lambda^-1 on Lambda's pattern, which the covariance call of this "
                               f"solver does not give for this structure (sparse mode: block columns of at most 8): {e}") from e
        return y_bar * (_logdet_weights(solver, lam, values) * sigma), None, None


def logdet(solver, lam, values: torch.Tensor) -> torch.Tensor:
    """log det M(values) on the block structure of ``lam``: a 0-dim float64 tensor, differentiable in ``values`` (module
    docstring; the backward pass factors again inside the covariance call)."""
    _check_solver(solver)
    _check_tensor(solver, values, "values", (int(lam.values.shape[0]),))
    _require_analysis(solver, lam)
    return _Logdet.apply(values, solver, lam)


# ---- the two substitutions one at a time: B M^-1 B^T, samples, whitening ----

def _check_rows(solver, lam, rows, name: str, n_max: int) -> None:
    n_scalars = int(lam.cumsum[-1])
    if isinstance(rows, torch.Tensor) and (rows.dim() != 2 or not 1 <= rows.shape[0] <= n_max):
        raise ValueError(f"{name} must be a tensor of the shape (k, n_scalars), 1 <= k <= {n_max}")
    _check_tensor(solver, rows, name, (rows.shape[0] if isinstance(rows, torch.Tensor) else 1, n_scalars))


def _factor(solver, values, zero) -> None:
    """Enqueues the factorization a solve makes, on the zero vector ``zero``: it leaves the kept factor."""
    solver.factor_solve_device_async(values.data_ptr(), zero.data_ptr())


def _factored_half(solver, values, rows, half: int, who: str):
    """Factors ``values`` and runs one substitution on a packed copy of ``rows``; waits.  Returns the copy."""
    out = rows.detach().clone(memory_format=torch.contiguous_format)
    v = values.detach()
    zero = torch.zeros(out.shape[1], dtype=torch.float64, device=out.device)

    def work():
        _factor(solver, v, zero)
        solver.solve_half_columns_device(out.data_ptr(), out.stride(0), out.shape[0], half)
    _enqueue(solver, work)
    if not solver.sync():
        raise torch.linalg.LinAlgError(f"{who}: the matrix is not positive definite")
    return out


class _QuadForm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, B, solver, lam):
        k, n = B.shape
        y = B.detach().clone(memory_format=torch.contiguous_format)
        v = values.detach()
        zero = torch.zeros(n, dtype=torch.float64, device=y.device)
        G = torch.empty((k, k), dtype=torch.float64, device=y.device)

        def forward_half():
            _factor(solver, v, zero)
            solver.solve_half_columns_device(y.data_ptr(), n, k, HALF_FORWARD)
            solver.gram_device(y.data_ptr(), n, k, y.data_ptr(), n, k, n, G.data_ptr(), k)
        _enqueue(solver, forward_half)
        b_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        if b_grad:                                  # X for backward; nobody to differentiate for: the forward half is all there is to do
            x = y.clone()
            _enqueue(solver, lambda: solver.solve_half_columns_device(x.data_ptr(), n, k, HALF_BACKWARD))
        if not solver.sync():
            raise torch.linalg.LinAlgError("quad_form: the matrix is not positive definite")
        if b_grad:
            ctx.solver, ctx.lam = solver, lam
            ctx.save_for_backward(values, x)
        return G

    @staticmethod
    @once_differentiable
    def backward(ctx, G_bar):
        values, x = ctx.saved_tensors
        solver = ctx.solver
        v_bar = None
        if ctx.needs_input_grad[0]:
            _require_analysis(solver, ctx.lam)      # (the outer products are on the handle's structure: it may have been given another since)
            v_bar = torch.empty_like(values)
            w = (G_bar @ x).contiguous()
            _enqueue(solver, lambda: solver.pattern_outer_sum_device(x.shape[0], x.data_ptr(), x.stride(0), w.data_ptr(),
                                                                     w.stride(0), v_bar.data_ptr(), -1.0, 0.0))
        B_bar = (G_bar + G_bar.transpose(0, 1)) @ x if ctx.needs_input_grad[1] else None
        return v_bar, B_bar, None, None


def quad_form(solver, lam, values: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """G = B M(values)^-1 B^T for B of the shape (k, n_scalars), k <= 48: a (k, k) tensor, bitwise symmetric, differentiable in
    ``values`` and ``B`` (module docstring).  Sparse mode, block columns of at most 8."""
    _check_solver(solver)
    _check_tensor(solver, values, "values", (int(lam.values.shape[0]),))
    _check_rows(solver, lam, B, "B", GRAM_MAX_COLUMNS)
    _require_analysis(solver, lam)
    return _QuadForm.apply(values, B, solver, lam)


def sample(solver, lam, values: torch.Tensor, Z: torch.Tensor) -> torch.Tensor:
    """Rows x = P^T L^-T z for the rows z of Z (k, n_scalars), L L^T = P M(values) P^T: standard normal z give samples of
    covariance M^-1.  NOT differentiable in ``values`` -- the derivative of the Cholesky factor is not built here --: the
    result is detached, and the call raises if ``values`` requires a gradient."""
    _check_solver(solver)
    _check_tensor(solver, values, "values", (int(lam.values.shape[0]),))
    _check_rows(solver, lam, Z, "Z", MAX_COLUMNS)
    if values.requires_grad:
        raise ValueError("sample: not differentiable in values (the derivative of the Cholesky factor is not built): detach them")
    _require_analysis(solver, lam)
    return _factored_half(solver, values, Z, HALF_BACKWARD, "sample")


def whiten(solver, lam, values: torch.Tensor, B: torch.Tensor):
    """(Y, perm): rows y = L^-1 P b for the rows b of B (k, n_scalars) -- whitened coordinates: |y|^2 = b^T M(values)^-1 b --
    in the factor's order, and the block permutation as an int64 CPU tensor: new block j is the caller's block perm[j].
    Detached, and raises if ``values`` requires a gradient, as ``sample``."""
    _check_solver(solver)
    _check_tensor(solver, values, "values", (int(lam.values.shape[0]),))
    _check_rows(solver, lam, B, "B", MAX_COLUMNS)
    if values.requires_grad:
        raise ValueError("whiten: not differentiable in values (the derivative of the Cholesky factor is not built): detach them")
    _require_analysis(solver, lam)
    Y = _factored_half(solver, values, B, HALF_FORWARD, "whiten")
    return Y, torch.from_numpy(solver.factor_structure()["perm"].astype(np.int64))
