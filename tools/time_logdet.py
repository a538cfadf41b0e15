"""Device-resident time of log det Lambda read from the factor in place (slampp_hip_logdet_device_async with b_reuse_factor = 1)
next to the factorization + solve that left the factor (slampp_hip_factor_solve_device_async), measured with device events
on the handle's stream after warm-up, in one process, on the benchmark's systems:

  C3         synth.pose_chain(100000)                 sparse mode: 600 000 scalar pivots through the table
  C4 venice  synth.ba(1000, 500000, mode="venice")    Schur mode, option schur_keep: 6 000 pivots of S and 500 000 landmarks

Also prints the time of the call that factors first (b_reuse_factor = 0) and the value itself.  None of these times is a
threshold: they are one-off measurements of a first implementation.

usage: python tools/time_logdet.py [--reps N] [--out FILE.json] [--only C3|venice]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from slam_plus_plus_amd import synth  # noqa: E402
from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP, CLinearSolver_Schur_HIP  # noqa: E402


def device_ms(solver, fn, reps):
    stream = torch.cuda.ExternalStream(solver.stream())
    fn()                                           # warm-up of this shape
    assert solver.sync()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(reps):
        fn()
    t1.record(stream)
    assert solver.sync()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def case(name, lam, reps):
    dev = torch.device("cuda:0")
    s = CLinearSolver_Schur_HIP(schur_keep=1) if lam.n_matrix_cut else CLinearSolver_HIP()
    s.SymbolicDecomposition_Blocky(lam)
    vals = torch.from_numpy(lam.values).to(dev)
    eta = torch.from_numpy(lam.rhs).to(dev)
    x = eta.clone()
    out = torch.zeros(2, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    t_fresh = device_ms(s, lambda: s.logdet_device(vals.data_ptr(), out.data_ptr() + 8, False), reps)
    t_solve = device_ms(s, lambda: (x.copy_(eta), s.factor_solve_device_async(vals.data_ptr(), x.data_ptr())), reps)
    t_reuse = device_ms(s, lambda: s.logdet_device(vals.data_ptr(), out.data_ptr(), True), reps)
    reused, fresh = out.cpu().tolist()
    return {"case": name, "n_bcols": lam.n_bcols, "n_scalars": lam.n_scalars, "factor_solve_ms": round(t_solve, 4),
            "logdet_reuse_ms": round(t_reuse, 4), "logdet_factoring_ms": round(t_fresh, 4), "logdet": reused,
            "reuse_minus_factoring": reused - fresh}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="C3 or venice")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_logdet: needs the GPU")
    results = []
    cases = [("C3", lambda: synth.pose_chain(n=100000)), ("venice", lambda: synth.ba(1000, 500000, mode="venice", seed=777))]
    for name, make in cases:
        if a.only and a.only != name:
            continue
        r = case(name, make(), a.reps)
        print(json.dumps(r), flush=True)
        results.append(r)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
