"""The robust kernels and the Levenberg-Marquardt loop with a robust edge set on 100 000 SE(3) poses (the graph of
tools/time_linearize.py and tools/time_lm.py: the edges of synth.pose_chain(100000), measurements = the expectations at the poses
plus noise; every 50th measurement is moved far enough for Huber to bite).

  kernels   each of slampp_hip_robust_weights_device_async (on the error's norm, which does not read Sigma^-1, and on the
            Mahalanobis distance), slampp_hip_robust_scale_device_async and slampp_hip_robust_chi_squared_device_async beside
            copy_*, a device-to-device copy of the bytes the call of that name reads and writes (the yardstick of DESIGN.md
            section 4.5, as tools/time_linearize.py measures linearize and chi2); windows of --reps calls between two events
  loops     a round of the device-decided loop three ways: plain (no robust kernel), reference (Huber on |err| / 0.3,
            SLAMPP_HIP_ROBUST_MODE_REFERENCE: CEdgePose3D) and loss (Huber on the Mahalanobis distance, SLAMPP_HIP_ROBUST_MODE_LOSS);
            a window is slampp_hip_lm_iterate_device_async(--reps) between two events on the solver's stream, from the same
            state with the same alpha

The ways alternate, window by window, --rounds times in one process, each after a warm-up of the very shape; per way the tool
prints the median and the spread (largest minus smallest window).  --count WAY: one begin and ten rounds of that way and nothing
else, for a kernel trace to count the dispatches of a round from.

usage: python tools/time_robust.py [--n POSES] [--reps N] [--rounds N] [--parts kernels,loops] [--ways plain,reference,loss] [--count WAY] [--out FILE.json]
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
from slam_plus_plus_amd import hip_solver as H  # noqa: E402
from slam_plus_plus_amd.hip_solver import CLambdaAssembly_HIP, CLevenbergMarquardt_HIP, CLinearSolver_HIP, EDGE_SE3, VERTEX_SE3  # noqa: E402


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
    ap.add_argument("--parts", default="kernels,loops")
    ap.add_argument("--ways", default="plain,reference,loss", help="the loops built and timed")
    ap.add_argument("--count", default=None, help="plain, reference or loss: ten rounds of that loop alone")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_robust: needs the GPU")
    has_robust = hasattr(CLambdaAssembly_HIP, "Set_Robust")                # (the plain loop also runs on a library from before)
    dev = torch.device("cuda:0")
    lam = synth.pose_chain(n=a.n)
    n_poses = lam.n_bcols
    cols = np.repeat(np.arange(n_poses), np.diff(lam.bcol_ptr))
    off = lam.brow_idx != cols
    v0, v1 = lam.brow_idx[off].astype(np.int64), cols[off].astype(np.int64)
    n_edges = len(v0)
    solver = CLinearSolver_HIP()
    stream, ours = torch.cuda.ExternalStream(solver.stream()), torch.cuda.current_stream(dev)

    def sync():
        assert solver.sync()
    rng = np.random.default_rng(7)
    i = np.arange(n_poses)
    state_h = np.stack([0.5 * i, 2 * np.sin(0.01 * i), 0.05 * i, 0.3 * np.sin(0.002 * i), 0.2 * np.cos(0.003 * i), 1.5 * np.sin(0.001 * i)], 1)
    state0 = torch.from_numpy(state_h.ravel()).to(dev)
    sigma = torch.from_numpy(np.tile((np.diag(40.0 + 3 * np.arange(6))).ravel(), n_edges)).to(dev)
    unary = (0, 10.0 * np.eye(6), None)
    specs = {"plain": None,
             "reference": dict(kernel=H.ROBUST_HUBER, basis=H.ROBUST_BASIS_ERROR_NORM, mode=H.ROBUST_MODE_REFERENCE, scale=0.3, param=1.345),
             "loss": dict(kernel=H.ROBUST_HUBER, basis=H.ROBUST_BASIS_MAHALANOBIS, mode=H.ROBUST_MODE_LOSS, scale=1.0, param=1.345)} \
        if has_robust else {"plain": None}
    specs = {w: s for w, s in specs.items() if w in ([a.count] if a.count else a.ways.split(","))}
    loops, z_dev = {}, None
    for way, spec in specs.items():
        asm = CLambdaAssembly_HIP(solver, lam, v0, v1, 6)
        sets = [dict(assembly=asm, edge_type=EDGE_SE3, measurement=torch.zeros(6 * n_edges, dtype=torch.float64, device=dev), sigma_inv=sigma)]
        if spec is not None:
            sets[0]["robust"] = spec
        lm = loops[way] = CLevenbergMarquardt_HIP(solver, lam, sets, [(VERTEX_SE3, 0, n_poses)], state0, unary, trace_capacity=a.reps)
        lm.asm, lm.z, lm.J0, lm.J1, lm.err = asm, lm._keep[1], lm._keep[5], lm._keep[6], lm._keep[7]
        if z_dev is None:                                                  # z = 0: err = -h; the measurements of every way
            torch.cuda.synchronize()
            asm.Linearize_device(EDGE_SE3, state0.data_ptr(), lm.z.data_ptr(), lm.J0.data_ptr(), lm.J1.data_ptr(), lm.err.data_ptr())
            sync()
            noise = rng.normal(0, 0.02, (n_edges, 6))
            noise[::50] += rng.normal(0, 0.5, (len(noise[::50]), 6))
            z_dev = -lm.err + torch.from_numpy(noise.ravel()).to(dev)
        lm.z.copy_(z_dev)
    torch.cuda.synchronize()
    first = next(iter(loops.values()))
    first.Begin(0.0, 1e-3, 0.0)
    ok, start, _ = first.Sync()
    assert ok
    alpha0 = float(start[H.LM_ALPHA])
    r = {"case": "C3" if a.n == 100000 else f"pose_chain({a.n})", "n_poses": n_poses, "n_edges": n_edges, "reps": a.reps, "rounds": a.rounds}
    if a.count:
        lm = loops[a.count]
        lm.Begin(alpha0, 0.0, 0.0)
        lm.Iterate(10)
        ok, scalars, _ = lm.Sync()
        print(json.dumps({"count": a.count, "rounds": int(scalars[H.LM_N_ROUNDS])}), flush=True)
        return
    ways = []
    if "kernels" in a.parts.split(",") and "loss" in loops and "reference" in loops:
        lm = loops["loss"]
        norm_asm = loops["reference"].asm
        out = torch.zeros(1, dtype=torch.float64, device=dev)
        lm.asm.Linearize_device(EDGE_SE3, state0.data_ptr(), lm.z.data_ptr(), lm.J0.data_ptr(), lm.J1.data_ptr(), lm.err.data_ptr())
        lm.asm.Robust_Weights_device(sigma.data_ptr(), lm.err.data_ptr())
        sync()
        r["edges_weighted_down"] = int((torch.as_tensor(_View(lm.asm.Robust_Weights_ptr(), n_edges), device=dev) < 1).sum())
        kernels = {"weights_error_norm": (lambda: norm_asm.Robust_Weights_device(0, lm.err.data_ptr()), 8 * 7 * n_edges),
                   "weights_mahalanobis": (lambda: lm.asm.Robust_Weights_device(sigma.data_ptr(), lm.err.data_ptr()), 8 * 43 * n_edges),
                   "scale": (lambda: lm.asm.Robust_Scale_device(lm.J0.data_ptr(), lm.J1.data_ptr(), lm.err.data_ptr()), 8 * (2 * 78 + 1) * n_edges),
                   "robust_chi2": (lambda: lm.asm.Robust_Chi2_device(sigma.data_ptr(), lm.err.data_ptr(), out.data_ptr()), 8 * 42 * n_edges),
                   "chi2": (lambda: lm.asm.Chi2_device(sigma.data_ptr(), lm.err.data_ptr(), 0, out.data_ptr()), 8 * 42 * n_edges)}
        src = torch.empty(max(b for _, b in kernels.values()) // 16, dtype=torch.float64, device=dev)
        dst = torch.empty_like(src)
        for name, (fn, n_bytes) in kernels.items():
            ways.append((name, fn, stream, sync, 1))
            ways.append(("copy_" + name, (lambda m=n_bytes // 16: dst[:m].copy_(src[:m])), ours, torch.cuda.synchronize, 1))
            r[name + "_bytes"] = n_bytes
    if "loops" in a.parts.split(","):
        for way, lm in loops.items():
            def window(lm=lm):
                lm.Iterate(a.reps)

            def prepare(lm=lm):
                lm.state.copy_(state0)
                torch.cuda.synchronize()
                lm.Begin(alpha0, 0.0, 0.0)
                sync()
            ways.append(("loop_" + way, window, stream, sync, a.reps, prepare))
    times = {w[0]: [] for w in ways}
    for _ in range(a.rounds):
        for name, fn, s, wait, per_call, *prepare in ways:
            for timed in (False, True):                                    # (a warm-up of the very shape first)
                if prepare:
                    prepare[0]()
                if timed:
                    times[name].append(window_ms(wait, s, fn, 1 if prepare else a.reps) / per_call)
                else:
                    fn()
                    wait()
    for name, t in times.items():
        r[name + "_ms"] = round(statistics.median(t), 4)
        r[name + "_spread_ms"] = round(max(t) - min(t), 4)
    for name in [k[:-6] for k in r if k.endswith("_bytes")]:
        r[name + "_GBps"] = round(r[name + "_bytes"] / (r[name + "_ms"] * 1e6), 1)
        r[name + "_over_copy"] = round(r[name + "_ms"] / r["copy_" + name + "_ms"], 2)
    for way, lm in loops.items():
        if "loop_" + way in times:
            s = lm.scalars_dev.cpu().numpy()
            r["loop_" + way + "_accepted_rejected_cost"] = (int(s[H.LM_N_ACCEPTED]), int(s[H.LM_N_REJECTED]), float(s[H.LM_LAST_ERROR]))
    print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(r, f, indent=1)


class _View:
    """n doubles of device memory as something torch.as_tensor takes."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2}


if __name__ == "__main__":
    main()
