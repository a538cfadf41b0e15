"""Ten Levenberg-Marquardt rounds on 100 000 SE(3) poses (the graph of tools/time_linearize.py: the edges of
synth.pose_chain(100000), measurements = the expectations at the poses plus noise), decided in two places:

  device   slampp_hip_lm_begin_device_async once, then slampp_hip_lm_iterate_device_async(rounds): every round enqueued, one wait
  host     the loop of INTEGRATION.md section 3a built from the calls the library had before the device-decided loop: per round
           linearize, assemble, a copy of eta, apply_damping with the host's alpha, factor_solve, three dot products (dx.dx,
           dx.eta, eta.eta), state_plus into a trial state, linearize and chi_squared there, one copy of the four scalars to
           pinned memory, slampp_hip_sync; then the rule of tests/lm_model.py in Python, and a copy trial -> state where it accepts

Both start every window from the same state with the same alpha and follow the same rule.  A window is timed with the host's
clock from the first enqueue to the return of the last wait (a device-side timing would leave out the very thing compared: the
time the device idles while the host decides).  The ways alternate, window by window, --windows times in one process, after a
warm-up window each; per way the tool prints the median per round and the spread (largest minus smallest window).

usage: python tools/time_lm.py [--n POSES] [--rounds N] [--windows N] [--ways device,host] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from slam_plus_plus_amd import synth  # noqa: E402
from slam_plus_plus_amd.hip_solver import (CLambdaAssembly_HIP, CLevenbergMarquardt_HIP, CLinearSolver_HIP, EDGE_SE3, LM_ALPHA,  # noqa: E402
                                           LM_N_ACCEPTED, LM_N_REJECTED, LM_LAST_ERROR, VERTEX_SE3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000, help="poses of the chain (the default is the benchmark's C3)")
    ap.add_argument("--rounds", type=int, default=10, help="LM rounds of a window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--ways", default="device,host")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_lm: needs the GPU")
    dev = torch.device("cuda:0")
    lam = synth.pose_chain(n=a.n)
    n, n_poses = lam.n_scalars, lam.n_bcols
    cols = np.repeat(np.arange(n_poses), np.diff(lam.bcol_ptr))
    off = lam.brow_idx != cols
    v0, v1 = lam.brow_idx[off].astype(np.int64), cols[off].astype(np.int64)
    n_edges = len(v0)
    solver = CLinearSolver_HIP()
    asm = CLambdaAssembly_HIP(solver, lam, v0, v1, 6)
    stream = torch.cuda.ExternalStream(solver.stream())
    rng = np.random.default_rng(7)
    i = np.arange(n_poses)
    state_h = np.stack([0.5 * i, 2 * np.sin(0.01 * i), 0.05 * i, 0.3 * np.sin(0.002 * i), 0.2 * np.cos(0.003 * i), 1.5 * np.sin(0.001 * i)], 1)
    state0 = torch.from_numpy(state_h.ravel()).to(dev)
    sigma = torch.from_numpy(np.tile((np.diag(40.0 + 3 * np.arange(6))).ravel(), n_edges)).to(dev)
    z = torch.zeros(6 * n_edges, dtype=torch.float64, device=dev)
    unary = (0, 10.0 * np.eye(6), None)
    lm = CLevenbergMarquardt_HIP(solver, lam, [dict(assembly=asm, edge_type=EDGE_SE3, measurement=z, sigma_inv=sigma)],
                                 [(VERTEX_SE3, 0, n_poses)], state0, unary, trace_capacity=a.rounds)
    z_dev = lm._keep[1]                                                    # (the loop's own measurement array)
    J0, J1, err = lm._keep[5], lm._keep[6], lm._keep[7]
    torch.cuda.synchronize()
    asm.Linearize_device(EDGE_SE3, state0.data_ptr(), z_dev.data_ptr(), J0.data_ptr(), J1.data_ptr(), err.data_ptr())   # z = 0: err = -h
    assert solver.sync()
    z_dev.copy_(-err + torch.from_numpy(rng.normal(0, 0.02, 6 * n_edges)).to(dev))
    torch.cuda.synchronize()
    # the start of every window: alpha and chi^2 of the start state, from one device-side begin
    lm.Begin(0.0, 1e-3, 0.0)
    ok, start, _ = lm.Sync()
    assert ok
    alpha0, chi2_0 = float(start[LM_ALPHA]), float(start[LM_LAST_ERROR])
    results = {}

    def device_window():
        lm.state.copy_(state0)
        torch.cuda.synchronize()
        lm.Begin(alpha0, 0.0, 0.0)                                         # (the host loop is handed alpha and chi^2 of the start too)
        assert solver.sync()
        t0 = time.perf_counter()
        lm.Iterate(a.rounds)
        ok, scalars, trace = lm.Sync()
        t = time.perf_counter() - t0
        assert ok
        results["device"] = (int(scalars[LM_N_ACCEPTED]), int(scalars[LM_N_REJECTED]), float(scalars[LM_LAST_ERROR]))
        return 1e3 * t / a.rounds

    # ---- the host-decided loop, from the calls of the commit before ----
    state, trial, dx, eta, values = lm.state, lm.trial, lm.dx, lm.eta, lm.values
    scalars_dev = torch.zeros(4, dtype=torch.float64, device=dev)
    scalars_host = torch.zeros(4, dtype=torch.float64).pin_memory()
    unary_host = (0, 10.0 * np.eye(6), None)

    def host_window():
        state.copy_(state0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        alpha, nu, last, n_acc, n_rej = alpha0, 2.0, chi2_0, 0, 0
        for _ in range(a.rounds):
            asm.Linearize_device(EDGE_SE3, state.data_ptr(), z_dev.data_ptr(), J0.data_ptr(), J1.data_ptr(), err.data_ptr())
            asm.Refresh_Lambda_device(J0.data_ptr(), J1.data_ptr(), sigma.data_ptr(), err.data_ptr(), 0, values.data_ptr(), eta.data_ptr(),
                                      *unary_host)
            with torch.cuda.stream(stream):
                dx.copy_(eta)
            solver.apply_damping_device_async(values.data_ptr(), alpha, 0, n_poses)
            solver.factor_solve_device_async(values.data_ptr(), dx.data_ptr())
            solver.dot_device(dx.data_ptr(), dx.data_ptr(), n, scalars_dev.data_ptr())
            solver.dot_device(dx.data_ptr(), eta.data_ptr(), n, scalars_dev.data_ptr() + 8)
            solver.dot_device(eta.data_ptr(), eta.data_ptr(), n, scalars_dev.data_ptr() + 16)
            solver.State_Plus_device(VERTEX_SE3, 0, n_poses, state.data_ptr(), dx.data_ptr(), trial.data_ptr())
            asm.Linearize_device(EDGE_SE3, trial.data_ptr(), z_dev.data_ptr(), J0.data_ptr(), J1.data_ptr(), err.data_ptr())
            asm.Chi2_device(sigma.data_ptr(), err.data_ptr(), 0, scalars_dev.data_ptr() + 24)
            with torch.cuda.stream(stream):
                scalars_host.copy_(scalars_dev, non_blocking=True)
            assert solver.sync()
            dx_dx, dx_eta, _, chi2 = scalars_host.tolist()
            rho = (last - chi2) / (alpha * dx_dx + dx_eta)
            if rho > 0:
                t = 2 * rho - 1
                alpha, nu, last, n_acc = alpha * max(1 / 3.0, 1 - t * t * t), 2.0, chi2, n_acc + 1
                with torch.cuda.stream(stream):
                    state.copy_(trial)
            else:
                alpha, nu, n_rej = alpha * nu, 2 * nu, n_rej + 1
        assert solver.sync()
        t = time.perf_counter() - t0
        results["host"] = (n_acc, n_rej, last)
        return 1e3 * t / a.rounds
    ways = [(w, {"device": device_window, "host": host_window}[w]) for w in a.ways.split(",")]
    times = {w: [] for w, _ in ways}
    for w, fn in ways:
        fn()                                                               # (warm-up of the very shapes)
    for _ in range(a.windows):
        for w, fn in ways:
            times[w].append(fn())
    r = {"case": "C3" if a.n == 100000 else f"pose_chain({a.n})", "n_poses": n_poses, "n_edges": n_edges, "rounds": a.rounds,
         "windows": a.windows}
    for w, t in times.items():
        r[w + "_ms_per_round"] = round(statistics.median(t), 4)
        r[w + "_spread_ms"] = round(max(t) - min(t), 4)
        r[w + "_accepted_rejected_chi2"] = results[w]
    print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


if __name__ == "__main__":
    main()
