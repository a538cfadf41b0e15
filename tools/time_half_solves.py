"""Device-resident time of the two substitutions of a k-column solve one at a time, and of the Gram product that goes with
the forward half, on the 100 000-pose SE(3) system of tools/time_c3.py (C3: synth.pose_chain(100000), sparse mode):

  columns    one slampp_hip_solve_columns_device_async call on a k-column array
  forward    one slampp_hip_solve_half_columns_device_async call, SLAMPP_HIP_HALF_FORWARD, on the same array
  backward   the same with SLAMPP_HIP_HALF_BACKWARD, on the forward half's result

for k = 1, 8 and 48: the halves should sum to about the whole, the copies between the interleaved workspace and the caller's
columns being what they add.  Then, on n_scalars x k of those numbers (600 000 rows) at k = 8 and 48:

  gram       slampp_hip_gram_device_async(Y, Y)
  copy       a device-to-device copy of the same bytes (the yardstick of DESIGN.md section 4.5)
  matmul     torch.matmul on the same arrays (Y Y^T for the row-major (k, n) tensor)

Everything is timed with device events on the handle's stream (matmul and the copy on torch's stream, with events there),
after a warm-up of the very shape, over windows of --reps calls; the ways alternate, window by window, --rounds times in
one process, so that whatever else the machine is doing meets all alike.  Per way the tool prints the median over the rounds
and the spread (largest minus smallest round).  The inputs are put back before every window.  Before anything is timed the
halves are checked to give the whole call's bits.

usage: python tools/time_half_solves.py [--n POSES] [--reps N] [--rounds N] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from slam_plus_plus_amd import synth  # noqa: E402
from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP, HALF_FORWARD, HALF_BACKWARD  # noqa: E402

KS = (1, 8, 48)
GRAM_KS = (8, 48)


def window_ms(sync, stream, fn, reps):
    """One timed window: reps calls of fn between two events on the stream, ended by a wait."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(reps):
        fn()
    t1.record(stream)
    sync()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def figures(times):
    out = {}
    for way, t in times.items():
        out[way + "_ms"] = round(statistics.median(t), 4)
        out[way + "_spread_ms"] = round(max(t) - min(t), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000, help="poses of the chain (the default is the benchmark's C3)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_half_solves: needs the GPU")
    dev = torch.device("cuda:0")
    lam = synth.pose_chain(n=a.n)
    n = lam.n_scalars
    solver = CLinearSolver_HIP()
    solver.SymbolicDecomposition_Blocky(lam)
    vals, x = torch.from_numpy(lam.values).to(dev), torch.from_numpy(lam.rhs).to(dev)
    assert solver.factor_solve_device(vals.data_ptr(), x.data_ptr())
    stream = torch.cuda.ExternalStream(solver.stream())

    def sync():
        assert solver.sync()
    rhs = torch.randn((max(KS), n), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    rhs[0] = torch.from_numpy(lam.rhs).to(dev)
    work, halfway = torch.empty_like(rhs), torch.empty_like(rhs)
    case = "C3" if a.n == 100000 else f"pose_chain({a.n})"
    results = []

    def report(r):
        print(json.dumps(r), flush=True)
        results.append(r)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)

    for k in KS:
        def columns():
            solver.solve_columns_device(work.data_ptr(), n, k)

        def forward():
            solver.solve_half_columns_device(work.data_ptr(), n, k, HALF_FORWARD)

        def backward():
            solver.solve_half_columns_device(work.data_ptr(), n, k, HALF_BACKWARD)

        # the halves give the whole call's bits at this size; what the backward half starts from is kept
        torch.cuda.synchronize()
        work.copy_(rhs)
        torch.cuda.synchronize()
        columns()
        sync()
        x_columns = work[:k].clone()
        work.copy_(rhs)
        torch.cuda.synchronize()
        forward()
        sync()
        halfway.copy_(work)
        torch.cuda.synchronize()
        backward()
        sync()
        same_bits = bool(torch.equal(x_columns, work[:k]))
        times = {"columns": [], "forward": [], "backward": []}
        for _ in range(a.rounds):
            for name, fn, start in (("columns", columns, rhs), ("forward", forward, rhs), ("backward", backward, halfway)):
                work.copy_(start)
                torch.cuda.synchronize()
                fn()                                                       # (warm-up of the very shape)
                sync()
                work.copy_(start)
                torch.cuda.synchronize()
                times[name].append(window_ms(sync, stream, fn, a.reps))
        r = {"case": case, "n_scalars": n, "k": k, "reps": a.reps, "rounds": a.rounds}
        r.update(figures(times))
        r["halves_over_columns"] = round((r["forward_ms"] + r["backward_ms"]) / r["columns_ms"], 3)
        r["halves_give_the_bits_of_columns"] = same_bits
        report(r)

    ours = torch.cuda.current_stream(dev)
    for k in GRAM_KS:
        y = halfway[:k]                                                    # (the forward half's result at k = 48)
        out = torch.empty((k, k), dtype=torch.float64, device=dev)
        copy_to = torch.empty_like(y)

        def gram():
            solver.gram_device(y.data_ptr(), n, k, y.data_ptr(), n, k, n, out.data_ptr(), k)

        def copy():
            copy_to.copy_(y)

        def matmul():
            torch.matmul(y, y.T)
        torch.cuda.synchronize()
        gram()
        sync()
        ref = torch.matmul(y, y.T)
        rel = float((out - ref).abs().max() / ref.abs().max())
        times = {"gram": [], "copy": [], "matmul": []}
        for _ in range(a.rounds):
            for name, fn, s, wait in (("gram", gram, stream, sync), ("copy", copy, ours, torch.cuda.synchronize),
                                      ("matmul", matmul, ours, torch.cuda.synchronize)):
                fn()
                wait()
                times[name].append(window_ms(wait, s, fn, a.reps))
        r = {"case": case, "n_rows": n, "k": k, "bytes": 8 * n * k, "reps": a.reps, "rounds": a.rounds}
        r.update(figures(times))
        r["gram_GBps_read"] = round(8 * n * k / (r["gram_ms"] * 1e6), 1)
        r["gram_over_copy"] = round(r["gram_ms"] / r["copy_ms"], 3)
        r["gram_rel_inf_against_matmul"] = rel
        report(r)


if __name__ == "__main__":
    main()
