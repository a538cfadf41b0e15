"""Device-resident time of k right-hand sides on the kept factor, two ways, on the 100 000-pose SE(3) system of tools/time_c3.py
(C3: synth.pose_chain(100000), sparse mode):

  columns   one slampp_hip_solve_columns_device_async call on a k-column array
  again     k calls of slampp_hip_solve_again_device_async, one per column of the same array

for k = 2, 8 and 48.  Both are timed with device events on the handle's stream, after a warm-up of the very shape, over
windows of --reps calls; the two ways alternate, window by window, --rounds times in one process, so that whatever else
the machine is doing meets both alike.  Per way and k the tool prints the median over the rounds and the spread (largest
minus smallest round), and whether the gap between the two medians is larger than the sum of the two spreads.  Before
anything is timed the two results are compared at the size that is timed (worst rel-inf over the columns).  The right-hand
sides are put back before every window: solutions fed back in as right-hand sides would drift in magnitude.

usage: python tools/time_solve_columns.py [--n POSES] [--reps N] [--rounds N] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from slam_plus_plus_amd import synth  # noqa: E402
from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP  # noqa: E402

KS = (2, 8, 48)


def window_ms(solver, stream, fn, reps):
    """One timed window: reps calls of fn between two events on the handle's stream, ended by a wait."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(reps):
        fn()
    t1.record(stream)
    assert solver.sync()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000, help="poses of the chain (the default is the benchmark's C3)")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_solve_columns: needs the GPU")
    dev = torch.device("cuda:0")
    lam = synth.pose_chain(n=a.n)
    n = lam.n_scalars
    solver = CLinearSolver_HIP()
    solver.SymbolicDecomposition_Blocky(lam)
    vals, x = torch.from_numpy(lam.values).to(dev), torch.from_numpy(lam.rhs).to(dev)
    assert solver.factor_solve_device(vals.data_ptr(), x.data_ptr())
    stream = torch.cuda.ExternalStream(solver.stream())
    rhs = torch.randn((max(KS), n), dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    rhs[0] = torch.from_numpy(lam.rhs).to(dev)
    work = torch.empty_like(rhs)
    results = []
    for k in KS:
        def columns():
            solver.solve_columns_device(work.data_ptr(), n, k)

        def again():
            for c in range(k):
                solver.solve_again_device(work.data_ptr() + 8 * c * n)

        # the two ways give the same solutions at this size
        torch.cuda.synchronize()
        work.copy_(rhs)
        torch.cuda.synchronize()
        columns()
        assert solver.sync()
        x_columns = work[:k].clone()
        work.copy_(rhs)
        torch.cuda.synchronize()
        again()
        assert solver.sync()
        rel = float(((x_columns - work[:k]).abs().amax(dim=1) / work[:k].abs().amax(dim=1)).max())
        times = {"columns": [], "again": []}
        for _ in range(a.rounds):
            for name, fn in (("columns", columns), ("again", again)):
                work.copy_(rhs)
                torch.cuda.synchronize()
                times[name].append(window_ms(solver, stream, fn, a.reps))
        med = {w: statistics.median(t) for w, t in times.items()}
        spread = {w: max(t) - min(t) for w, t in times.items()}
        r = {"case": "C3" if a.n == 100000 else f"pose_chain({a.n})", "n_scalars": n, "k": k, "reps": a.reps, "rounds": a.rounds,
             "columns_ms": round(med["columns"], 4), "columns_spread_ms": round(spread["columns"], 4),
             "again_ms": round(med["again"], 4), "again_spread_ms": round(spread["again"], 4),
             "again_over_columns": round(med["again"] / med["columns"], 3),
             "columns_wins_beyond_spread": med["again"] - med["columns"] > spread["columns"] + spread["again"],
             "worst_rel_inf_between_the_two": rel}
        print(json.dumps(r), flush=True)
        results.append(r)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
