"""Device-resident time of the two ends of a Gauss-Newton iteration on 100 000 SE(3) poses with the edges of
synth.pose_chain(100000) (C3's graph: 99 999 odometry edges and 1 999 loop closures), beside the step they frame:

  linearize    one slampp_hip_linearize_device_async call (SLAMPP_HIP_EDGE_SE3): gathers 18 doubles an edge, writes 78
  state_plus   one slampp_hip_state_plus_device_async call (SLAMPP_HIP_VERTEX_SE3) on all block columns, in place
  chi2         one slampp_hip_chi_squared_device_async call
  copy_*       a device-to-device copy of the bytes the call of that name reads and writes (the yardstick of DESIGN.md section 4.5)
  solve_step   slampp_hip_assemble_device_async + slampp_hip_factor_solve_device_async of the same handle

The poses follow a gently turning chain; the measurements are the expectations at those poses plus noise (formed on the device:
a linearize call with z = 0 returns err = -h), so the system the step solves is the one a converging loop meets.  Everything
is timed with device events on the handle's stream (the copies on torch's stream, with events there), after a warm-up of the
very shape, over windows of --reps calls; the ways alternate, window by window, --rounds times in one process.  Per way the tool
prints the median over the rounds and the spread (largest minus smallest round).

usage: python tools/time_linearize.py [--n POSES] [--reps N] [--rounds N] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from slam_plus_plus_amd import synth  # noqa: E402
from slam_plus_plus_amd.hip_solver import CLambdaAssembly_HIP, CLinearSolver_HIP, EDGE_SE3, VERTEX_SE3  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000, help="poses of the chain (the default is the benchmark's C3)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_linearize: needs the GPU")
    dev = torch.device("cuda:0")
    lam = synth.pose_chain(n=a.n)
    n, n_poses = lam.n_scalars, lam.n_bcols
    cols = np.repeat(np.arange(n_poses), np.diff(lam.bcol_ptr))
    off = lam.brow_idx != cols
    v0, v1 = lam.brow_idx[off].astype(np.int64), cols[off].astype(np.int64)
    n_edges = len(v0)
    solver = CLinearSolver_HIP()
    asm = CLambdaAssembly_HIP(solver, lam, v0, v1, 6)
    stream, ours = torch.cuda.ExternalStream(solver.stream()), torch.cuda.current_stream(dev)

    def sync():
        assert solver.sync()
    rng = np.random.default_rng(7)
    i = np.arange(n_poses)
    state_h = np.stack([0.5 * i, 2 * np.sin(0.01 * i), 0.05 * i, 0.3 * np.sin(0.002 * i), 0.2 * np.cos(0.003 * i), 1.5 * np.sin(0.001 * i)], 1)
    state = torch.from_numpy(state_h.ravel()).to(dev)
    sigma = torch.from_numpy(np.tile((np.diag(40.0 + 3 * np.arange(6))).ravel(), n_edges)).to(dev)
    z = torch.zeros(6 * n_edges, dtype=torch.float64, device=dev)
    J0, J1 = torch.empty(36 * n_edges, dtype=torch.float64, device=dev), torch.empty(36 * n_edges, dtype=torch.float64, device=dev)
    err = torch.empty(6 * n_edges, dtype=torch.float64, device=dev)
    values, eta = torch.empty(lam.values.shape[0], dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
    chi2 = torch.zeros(1, dtype=torch.float64, device=dev)
    dx = torch.from_numpy(rng.normal(0, 1e-3, n)).to(dev)
    unary = (0, 10.0 * np.eye(6), np.zeros(6))

    def linearize():
        asm.Linearize_device(EDGE_SE3, state.data_ptr(), z.data_ptr(), J0.data_ptr(), J1.data_ptr(), err.data_ptr())

    def state_plus():
        solver.State_Plus_device(VERTEX_SE3, 0, n_poses, state.data_ptr(), dx.data_ptr(), state.data_ptr())

    def chi_squared():
        asm.Chi2_device(sigma.data_ptr(), err.data_ptr(), 0, chi2.data_ptr())

    def solve_step():
        asm.Refresh_Lambda_device(J0.data_ptr(), J1.data_ptr(), sigma.data_ptr(), err.data_ptr(), 0, values.data_ptr(), eta.data_ptr(),
                                  *unary)
        solver.factor_solve_device_async(values.data_ptr(), eta.data_ptr())
    torch.cuda.synchronize()
    linearize()                                                            # z = 0: err = -h
    sync()
    z.copy_(-err + torch.from_numpy(rng.normal(0, 0.02, 6 * n_edges)).to(dev))
    torch.cuda.synchronize()
    linearize()
    chi_squared()
    solve_step()
    sync()
    bytes_of = {"linearize": 8 * (3 * n_edges + 18 * n_edges + 78 * n_edges),    # offsets and vertex, states and z, outputs
                "state_plus": 8 * (3 * n + n_poses), "chi2": 8 * 42 * n_edges}
    src = torch.empty(max(bytes_of.values()) // 16, dtype=torch.float64, device=dev)
    dst = torch.empty_like(src)
    ways = [("linearize", linearize, stream, sync), ("state_plus", state_plus, stream, sync), ("chi2", chi_squared, stream, sync),
            ("solve_step", solve_step, stream, sync)]
    for name, n_bytes in bytes_of.items():
        ways.append(("copy_" + name, (lambda m=n_bytes // 16: dst[:m].copy_(src[:m])), ours, torch.cuda.synchronize))
    times = {name: [] for name, _, _, _ in ways}
    state0 = state.clone()
    for _ in range(a.rounds):
        for name, fn, s, wait in ways:
            state.copy_(state0)
            torch.cuda.synchronize()
            fn()                                                           # (warm-up of the very shape)
            wait()
            times[name].append(window_ms(wait, s, fn, a.reps))
    r = {"case": "C3" if a.n == 100000 else f"pose_chain({a.n})", "n_poses": n_poses, "n_edges": n_edges, "reps": a.reps,
         "rounds": a.rounds, "chi2": float(chi2)}
    for name, t in times.items():
        r[name + "_ms"] = round(statistics.median(t), 4)
        r[name + "_spread_ms"] = round(max(t) - min(t), 4)
    for name, n_bytes in bytes_of.items():
        r[name + "_bytes"] = n_bytes
        r[name + "_GBps"] = round(n_bytes / (r[name + "_ms"] * 1e6), 1)
        r[name + "_over_copy"] = round(r[name + "_ms"] / r["copy_" + name + "_ms"], 2)
    print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
