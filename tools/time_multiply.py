"""Device-resident times of the product y = alpha Lambda x + beta y (slampp_hip_multiply_device_async), of the re-solve on
the kept factor (slampp_hip_solve_again_device_async) and of one step of iterative refinement
(slampp_hip_refine_device_async), measured with device events on the handle's stream after warm-up, in one process:

  C3         synth.pose_chain(100000)                 sparse mode: short rows only
  C4 venice  synth.ba(1000, 500000, mode="venice")    Schur mode, option schur_keep: camera rows of thousands of blocks (chunks)
  C4 band    synth.ba(1000, 500000, mode="band")      Schur mode, option schur_keep

The product reads every stored value once (off-diagonal blocks twice: once for either block row), x and y; its GB/s is
reported over the bytes of the values array alone, the figure a caller can compare with the 8 TB/s of HBM.  None of
these times is a threshold: they are one-off measurements of a first implementation.

usage: python tools/time_multiply.py [--reps N] [--out FILE.json] [--only C3|venice|band]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
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
    n = lam.n_scalars
    vals = torch.from_numpy(lam.values).to(dev)
    eta = torch.from_numpy(lam.rhs).to(dev)
    x = eta.clone()
    y = torch.empty_like(eta)
    rhs = eta.clone()
    resid = torch.zeros(2, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    t_solve = device_ms(s, lambda: (x.copy_(eta), s.factor_solve_device_async(vals.data_ptr(), x.data_ptr())), reps)
    t_mul = device_ms(s, lambda: s.multiply_device(vals.data_ptr(), x.data_ptr(), y.data_ptr(), 1.0, 0.0), reps)
    t_again = device_ms(s, lambda: s.solve_again_device(rhs.data_ptr()), reps)
    t_refine = device_ms(s, lambda: s.refine_device(vals.data_ptr(), eta.data_ptr(), x.data_ptr(), 1, 0), reps)
    s.refine_device(vals.data_ptr(), eta.data_ptr(), x.data_ptr(), 1, resid.data_ptr())
    assert s.sync()
    ref = lam.to_scipy() @ x.cpu().numpy() if n <= 700_000 else None
    s.multiply_device(vals.data_ptr(), x.data_ptr(), y.data_ptr(), 1.0, 0.0)
    assert s.sync()
    n_bytes = 8.0 * lam.values.shape[0]
    rows = np.diff(lam.bcol_ptr).astype(np.int64)
    np.add.at(rows, lam.brow_idx[lam.brow_idx != np.repeat(np.arange(lam.n_bcols), np.diff(lam.bcol_ptr))], 1)
    return {
        "case": name, "n_bcols": lam.n_bcols, "n_scalars": n, "values_bytes": n_bytes, "longest_block_row": int(rows.max()),
        "factor_solve_ms": round(t_solve, 4),
        "multiply_ms": round(t_mul, 4), "multiply_GBps_over_values": round(n_bytes / (t_mul * 1e-3) / 1e9, 1),
        "solve_again_ms": round(t_again, 4), "refine_one_step_ms": round(t_refine, 4),
        "residual_inf_before_after": resid.cpu().numpy().tolist(),
        "multiply_vs_scipy_rel_inf": None if ref is None else float(np.abs(y.cpu().numpy() - ref).max() / np.abs(ref).max()),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="C3, venice or band")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_multiply: needs the GPU")
    results = []
    cases = [("C3", lambda: synth.pose_chain(n=100000)), ("venice", lambda: synth.ba(1000, 500000, mode="venice", seed=777)),
             ("band", lambda: synth.ba(1000, 500000, k=4, mode="band", seed=777))]
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
