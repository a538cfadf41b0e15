"""Device-resident times of the covariance calls beyond the block diagonal (slampp_hip_marginals_pattern,
slampp_hip_marginal_columns), measured with device events on the handle's stream after warm-up, in one process:

  (a) marginals_pattern next to marginals (block diagonal), both factoring the values;
  (b) the last block column from the factor in place (k = d);
  (c) 8 block columns from the factor in place (k = 48 for 6 x 6 blocks);
  (d) the same columns the old way, one slampp_hip_solve_again per unit vector (host clock; includes PCIe both ways).

Sizes: C3 = synth.pose_chain(100000) and a C2-like synth.sphere(50, 50) whose default plan has a dense top.  Bytes each
call must move are computed from the plan: the factor L once (scalar nonzeros of L x 8 B), the n_scalars x k workspace
(written once and read once by the backward substitution), the n_scalars x k output; for the pattern the output and the
same number of doubles of Z read.  "share of HBM peak" = those bytes / time / 8.0 TB/s (the spec peak), a floor on what
the hardware could do for that traffic, not a kernel's utilisation.  Per-kernel times: run this under
rocprofv3 --kernel-trace --stats in a separate run.

usage: python tools/time_covariance.py [--reps N] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from slam_plus_plus_amd import synth  # noqa: E402
from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP, _ptr  # noqa: E402

HBM_PEAK = 8.0e12   # bytes/s, MI355X spec


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
    s = CLinearSolver_HIP()
    s.SymbolicDecomposition_Blocky(lam)
    lib, h = s._lib, s._h
    st, plan = s.stats(), s.plan()
    n, d = lam.n_scalars, int(lam.cumsum[1])
    vals = torch.from_numpy(lam.values).to(dev)
    diag = torch.empty(lam.n_bcols * d * d, dtype=torch.float64, device=dev)
    patt = torch.empty_like(vals)
    last = np.array([lam.n_bcols - 1], dtype=np.int64)
    eight = np.linspace(0, lam.n_bcols - 1, 8).astype(np.int64)
    eight[-1] = lam.n_bcols - 1
    out = torch.empty(n * 48, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()

    def rc(x):
        assert x == 0, s._error()

    t_diag = device_ms(s, lambda: rc(lib.slampp_hip_marginals_device_async(h, vals.data_ptr(), diag.data_ptr())), reps)
    t_patt = device_ms(s, lambda: rc(lib.slampp_hip_marginals_pattern_device_async(h, vals.data_ptr(), patt.data_ptr())), reps)
    t_last = device_ms(s, lambda: rc(lib.slampp_hip_marginal_columns_device_async(h, None, 1, _ptr(last), out.data_ptr())), reps)
    t_k48 = device_ms(s, lambda: rc(lib.slampp_hip_marginal_columns_device_async(h, None, 8, _ptr(eight), out.data_ptr())), reps)
    X48 = out.view(48, n).cpu().numpy().T
    # (d) the old way: one solve_again per unit vector, the factor in place (host clock, PCIe included)
    cs = lam.cumsum

    def old_way(cols):
        X = np.empty((n, sum(int(cs[c + 1] - cs[c]) for c in cols)))
        j = 0
        for c in cols:
            for r in range(int(cs[c]), int(cs[c + 1])):
                e = np.zeros(n)
                e[r] = 1.0
                assert s.Solve_Again(e)
                X[:, j] = e
                j += 1
        return X
    old_way(last[:1])                                  # warm-up
    t0 = time.perf_counter()
    old_way(last)
    t_old_last = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    X_old = old_way(eight)
    t_old_k48 = (time.perf_counter() - t0) * 1e3
    agree = float(np.abs(X48 - X_old).max() / np.abs(X_old).max())

    l_bytes = 8.0 * st["l_nnz"]

    def bw(bytes_, ms):
        return {"bytes": bytes_, "ms": round(ms, 4), "bytes_per_s": bytes_ / (ms * 1e-3),
                "share_of_hbm_peak": bytes_ / (ms * 1e-3) / HBM_PEAK}
    res = {
        "case": name, "n_bcols": lam.n_bcols, "n_scalars": n, "dense_dim": plan["dense_dim"], "n_stages": st["n_stages"],
        "etree_height": st["etree_height"], "l_nnz": st["l_nnz"],
        "a_marginals_ms": round(t_diag, 4), "a_marginals_pattern_ms": round(t_patt, 4),
        "b_last_column_k%d" % d: bw(l_bytes + 3 * 8.0 * n * d, t_last),
        "c_8_columns_k48": bw(l_bytes + 3 * 8.0 * n * 48, t_k48),
        "d_old_way_last_column_ms_incl_pcie": round(t_old_last, 3), "d_old_way_8_columns_ms_incl_pcie": round(t_old_k48, 3),
        "columns_vs_old_way_rel_inf": agree,
        "pattern_gather_bytes": 2 * 8.0 * lam.values.shape[0],
    }
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="C3 or C2")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_covariance: needs the GPU")
    results = []
    cases = [("C3", lambda: synth.pose_chain(n=100000)), ("C2", lambda: synth.sphere(50, 50))]
    for name, make in cases:
        if a.only and a.only != name:
            continue
        r = case(name, make(), a.reps)
        print(json.dumps(r))
        results.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
