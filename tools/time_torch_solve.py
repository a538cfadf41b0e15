"""Device times of the differentiable solve (slam_plus_plus_amd/torch_solve.py) and of the outer product on Lambda's
pattern that its backward pass ends with (slampp_hip_pattern_outer_device_async), measured with device events on the
handle's stream, one pair per step, after warm-up, in one process; medians over the steps:

  C3         synth.pose_chain(100000)                 sparse mode
  C4 venice  synth.ba(1000, 500000, mode="venice")    Schur mode, option schur_keep

  kernel     the outer product alone (alpha = -1, beta = 0): it writes 8 n_values bytes
  copy       a device-to-device copy_ of n_values doubles on the same stream: the store rate this session can reach
  forward    solve(): slampp_hip_factor_solve_device_async on a clone of eta (the wait for the device that follows it is
             outside the events)
  bwd kept   backward on the kept factor: the re-solve of x_bar and the kernel
  bwd again  backward after another forward on the same handle took the factor: a factorization, the solve and the kernel

GB/s are over the 8 n_values bytes written (the copy reads as many again).  None of these times is a threshold.

usage: python tools/time_torch_solve.py [--steps N] [--out FILE.txt] [--only C3|venice]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from slam_plus_plus_amd import synth  # noqa: E402
from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP, CLinearSolver_Schur_HIP  # noqa: E402
from slam_plus_plus_amd.torch_solve import solve  # noqa: E402

WARMUP = 3


def median_ms(solver, step, steps, before=None):
    """Median device time of step() over ``steps`` runs after WARMUP: an event pair on the solver's stream around each
    (before(), where given, runs ahead of every step, outside its events)."""
    stream = torch.cuda.ExternalStream(solver.stream())
    pairs = []
    for i in range(WARMUP + steps):
        if before is not None:
            before()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(stream)
        step()
        t1.record(stream)
        if i >= WARMUP:
            pairs.append((t0, t1))
    assert solver.sync()
    torch.cuda.current_stream().synchronize()
    return statistics.median(t0.elapsed_time(t1) for t0, t1 in pairs)


def case(name, lam, steps):
    dev = torch.device("cuda:0")
    solver = CLinearSolver_Schur_HIP(schur_keep=1) if lam.n_matrix_cut else CLinearSolver_HIP()
    n_values = lam.values.shape[0]
    values = torch.from_numpy(lam.values).to(dev).requires_grad_(True)
    eta = torch.from_numpy(lam.rhs).to(dev).requires_grad_(True)
    w = torch.ones(lam.n_scalars, dtype=torch.float64, device=dev)
    state = {}

    def forward():
        state["x"] = solve(solver, lam, values, eta)

    def two_forwards():
        forward()
        solve(solver, lam, values, eta)            # ... which takes the factor away from state["x"]

    def backward():
        values.grad = eta.grad = None
        torch.autograd.backward(state["x"], w)

    forward()                                      # the analysis
    t_forward = median_ms(solver, forward, steps)
    t_kept = median_ms(solver, backward, steps, before=forward)
    assert solver.n_backward_refactorizations == 0
    t_again = median_ms(solver, backward, steps, before=two_forwards)
    assert solver.n_backward_refactorizations == WARMUP + steps
    # the kernel alone and the copy, on vectors of the right size
    g, x = w.clone(), state["x"].detach()
    out, src = torch.empty(n_values, dtype=torch.float64, device=dev), values.detach()
    t_kernel = median_ms(solver, lambda: solver.pattern_outer_device(g.data_ptr(), x.data_ptr(), out.data_ptr(), -1.0, 0.0), steps)
    stream = torch.cuda.ExternalStream(solver.stream())

    def copy():
        with torch.cuda.stream(stream):
            out.copy_(src)
    t_copy = median_ms(solver, copy, steps)
    n_bytes = 8.0 * n_values
    return {"case": name, "n_scalars": lam.n_scalars, "n_values": n_values, "kernel_ms": t_kernel,
            "kernel_GBps": n_bytes / t_kernel / 1e6, "copy_ms": t_copy, "copy_GBps": n_bytes / t_copy / 1e6,
            "kernel_over_copy": t_kernel / t_copy, "forward_ms": t_forward, "backward_kept_ms": t_kept,
            "backward_again_ms": t_again, "kept_over_forward": t_kept / t_forward}


def table(results, steps):
    lines = [f"tools/time_torch_solve.py: medians of {steps} steps after {WARMUP} of warm-up, device events on the solver's stream",
             f"{'case':<8}{'n_scalars':>11}{'n_values':>12}{'kernel ms':>11}{'GB/s':>8}{'copy ms':>10}{'GB/s':>8}{'k/copy':>8}"
             f"{'forward ms':>12}{'bwd kept ms':>13}{'bwd again ms':>14}{'kept/fwd':>10}"]
    for r in results:
        lines.append(f"{r['case']:<8}{r['n_scalars']:>11}{r['n_values']:>12}{r['kernel_ms']:>11.4f}{r['kernel_GBps']:>8.0f}"
                     f"{r['copy_ms']:>10.4f}{r['copy_GBps']:>8.0f}{r['kernel_over_copy']:>8.2f}{r['forward_ms']:>12.3f}"
                     f"{r['backward_kept_ms']:>13.3f}{r['backward_again_ms']:>14.3f}{r['kept_over_forward']:>10.2f}")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="C3 or venice")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_torch_solve: needs the GPU")
    results = []
    cases = [("C3", lambda: synth.pose_chain(n=100000)), ("venice", lambda: synth.ba(1000, 500000, mode="venice", seed=777))]
    for name, make in cases:
        if a.only and a.only != name:
            continue
        results.append(case(name, make(), a.steps))
        text = table(results, a.steps)
        print(text, flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
