"""Device-resident times of the Schur-mode covariance calls beyond the block diagonal
(slampp_hip_schur_marginals_pattern, slampp_hip_schur_marginal_columns), measured with device events on the handle's stream
after warm-up, in one process:

  (a) schur_marginals (block diagonal) next to schur_marginals_pattern, both factoring the values;
  (b) one camera column from the factor in place (k = dc);
  (c) eight camera columns from the factor in place (k = 8 dc);
  (d) one landmark column from the factor in place (k = dp).

Sizes: C4 band and C4 Venice (synth.ba(1000, 500 000, mode=...)).  Bytes each call must move at least: for the pattern, its
output (Lambda's values), W and C^-1 once and Lambda's values once (read by the assembly); for the columns, W once (the
landmark rows), the n_scalars x k output.  "share of HBM peak" = those bytes / time / 8.0 TB/s (the spec peak), a floor on
what the hardware could do for that traffic, not a kernel's utilisation.  Per-kernel times: run this under
rocprofv3 --kernel-trace --stats in a separate run.

usage: python tools/time_schur_covariance.py [--reps N] [--only band|venice] [--out FILE.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from slam_plus_plus_amd import synth  # noqa: E402
from slam_plus_plus_amd.hip_solver import CLinearSolver_Schur_HIP, _ptr  # noqa: E402

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
    s = CLinearSolver_Schur_HIP()
    s.SymbolicDecomposition_Blocky(lam, True)
    lib, h = s._lib, s._h
    nc = lam.n_matrix_cut
    n, dc, dp = lam.n_scalars, int(lam.cumsum[1]), int(lam.cumsum[nc + 1] - lam.cumsum[nc])
    n_pts, n_obs = lam.n_bcols - nc, lam.n_blocks - lam.n_bcols - (int(lam.bcol_ptr[nc]) - nc)
    vals = torch.from_numpy(lam.values).to(dev)
    cams = torch.empty(nc * dc * dc, dtype=torch.float64, device=dev)
    pts = torch.empty(n_pts * dp * dp, dtype=torch.float64, device=dev)
    patt = torch.empty_like(vals)
    one = np.array([nc // 2], dtype=np.int64)
    eight = np.linspace(0, nc - 1, 8).astype(np.int64)
    lm = np.array([nc + n_pts // 2], dtype=np.int64)
    out = torch.empty(n * 8 * dc, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()

    def rc(x):
        assert x == 0, s._error()

    t_diag = device_ms(s, lambda: rc(lib.slampp_hip_schur_marginals_device_async(h, vals.data_ptr(), cams.data_ptr(),
                                                                                  pts.data_ptr())), reps)
    t_patt = device_ms(s, lambda: rc(lib.slampp_hip_schur_marginals_pattern_device_async(h, vals.data_ptr(),
                                                                                         patt.data_ptr())), reps)
    t_one = device_ms(s, lambda: rc(lib.slampp_hip_schur_marginal_columns_device_async(h, None, 1, _ptr(one),
                                                                                       out.data_ptr())), reps)
    t_eight = device_ms(s, lambda: rc(lib.slampp_hip_schur_marginal_columns_device_async(h, None, 8, _ptr(eight),
                                                                                         out.data_ptr())), reps)
    t_lm = device_ms(s, lambda: rc(lib.slampp_hip_schur_marginal_columns_device_async(h, None, 1, _ptr(lm),
                                                                                      out.data_ptr())), reps)
    w_bytes = 8.0 * (n_obs * dc * dp + n_pts * dp * dp)      # W and C^-1

    def bw(bytes_, ms):
        return {"bytes": bytes_, "ms": round(ms, 4), "bytes_per_s": bytes_ / (ms * 1e-3),
                "share_of_hbm_peak": bytes_ / (ms * 1e-3) / HBM_PEAK}
    v_bytes = 8.0 * lam.values.shape[0]
    return {
        "case": name, "n_cams": nc, "n_points": n_pts, "n_observations": n_obs, "n_scalars": n,
        "a_schur_marginals_ms": round(t_diag, 4),
        "a_schur_marginals_pattern": bw(2 * v_bytes + w_bytes, t_patt),
        "a_pattern_over_marginals": round(t_patt / t_diag, 3),
        "b_one_camera_column_k%d" % dc: bw(w_bytes + 8.0 * n * dc, t_one),
        "c_8_camera_columns_k%d" % (8 * dc): bw(w_bytes + 8.0 * n * 8 * dc, t_eight),
        "d_one_landmark_column_k%d" % dp: bw(w_bytes + 8.0 * n * dp, t_lm),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="band or venice")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_schur_covariance: needs the GPU")
    results = []
    for mode in ("band", "venice"):
        if a.only and a.only != mode:
            continue
        r = case("C4_" + mode, synth.ba(1000, 500_000, mode=mode), a.reps)
        print(json.dumps(r), flush=True)
        results.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
