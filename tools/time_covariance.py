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

With --pairs, instead: blocks at arbitrary pairs (slampp_hip_marginal_blocks) next to the only other route to them,
whole block columns, on C3 with the values in HBM and the factor in place:

  (a) marginal_blocks for 32 seeded random pairs;
  (b) marginal_columns(values = NULL) on those pairs' distinct columns (the blocks are then rows picked out of n_scalars x k);
  (c) the last pose against 64 candidates: marginal_blocks for the 64 pairs, next to marginal_columns([last]), whose single
      column holds all of them.

Each time is the median of --repeats windows of --reps calls between two device events; the host's list building lies
inside the window (the device waits for it), and is also given alone (host clock around one call, enqueue only).  Device
bytes each route allocates are computed from the shapes: the n_scalars x 48 workspace both share, and each route's output.

With --schur-pairs, the same for BA systems in Schur mode (slampp_hip_schur_marginal_blocks next to
slampp_hip_schur_marginal_columns(values = NULL)), on the BA benchmark configuration (1000 cameras x 500 000 points,
Venice-style visibility: the reduced system is inverted densely) and on the band configuration whose reduced system is
factored by the sparse block path:

  (a) schur_marginal_blocks for 32 seeded mixed pairs (cameras and landmarks in every combination);
  (b) schur_marginal_columns on those pairs' distinct columns;
  (c) one camera against 64 candidate landmarks, both ways: the 64 pairs, next to the camera's one block column.

What its figures cover: "host_enqueue_ms" is the host clock around one whole enqueue-only call -- the checks, the list
building (pair records, column sets, the planner, the passes' forward lists), the enqueue of the uploads and of every
launch -- so it bounds the list building from above; the library does not time that part alone.
"handle_device_bytes" is slampp_hip_get_stats' device_bytes of the handle after the analysis, after the first blocks call
and after the columns calls: it counts everything the handle holds on the device, the Schur state's W, C^-1, tables and
right-hand-side buffer, the reduced system's factor or dense inverse, and the inner solver's covariance workspace
(n_scalars_S x 48 doubles) and pair lists included -- the differences are what each route allocates on top; the caller's
own output buffers are "device_bytes_output".  Per-kernel times: a run of its own under rocprofv3 --kernel-trace --stats
(--only picks the configuration).

usage: python tools/time_covariance.py [--reps N] [--out FILE.json] [--pairs | --schur-pairs [--repeats M]]
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
from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP, CLinearSolver_Schur_HIP, _ptr  # noqa: E402

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


def pairs_case(name, lam, reps, repeats):
    dev = torch.device("cuda:0")
    s = CLinearSolver_HIP()
    s.SymbolicDecomposition_Blocky(lam)
    lib, h = s._lib, s._h
    st, plan = s.stats(), s.plan()
    n, nb, d = lam.n_scalars, lam.n_bcols, int(lam.cumsum[1])
    vals = torch.from_numpy(lam.values).to(dev)
    rng = np.random.default_rng(17)
    rows32, cols32 = (np.ascontiguousarray(rng.integers(0, nb, 32), dtype=np.int64) for _ in range(2))
    distinct = np.unique(np.concatenate([rows32, cols32])).astype(np.int64)
    last = np.array([nb - 1], dtype=np.int64)
    cand = np.ascontiguousarray(np.sort(rng.choice(nb - 1, size=64, replace=False)), dtype=np.int64)
    last64 = np.full(64, nb - 1, dtype=np.int64)
    blocks = torch.empty(64 * d * d, dtype=torch.float64, device=dev)
    out = torch.empty(n * d * len(distinct), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()

    def rc(x):
        assert x == 0, s._error()

    rc(lib.slampp_hip_marginal_blocks_device_async(h, vals.data_ptr(), 32, _ptr(rows32), _ptr(cols32), blocks.data_ptr()))
    assert s.sync()                                                       # the factor is in place from here on
    legs = {
        "a_blocks_32_pairs": lambda: rc(lib.slampp_hip_marginal_blocks_device_async(h, None, 32, _ptr(rows32), _ptr(cols32), blocks.data_ptr())),
        "b_columns_of_32_pairs": lambda: rc(lib.slampp_hip_marginal_columns_device_async(h, None, len(distinct), _ptr(distinct), out.data_ptr())),
        "c_blocks_last_vs_64": lambda: rc(lib.slampp_hip_marginal_blocks_device_async(h, None, 64, _ptr(cand), _ptr(last64), blocks.data_ptr())),
        "c_columns_last": lambda: rc(lib.slampp_hip_marginal_columns_device_async(h, None, 1, _ptr(last), out.data_ptr())),
    }
    times = {k: [] for k in legs}
    for _ in range(repeats):                                              # the legs alternate: drift hits all of them alike
        for k, fn in legs.items():
            times[k].append(device_ms(s, fn, reps))
    host = {}
    for k, fn in legs.items():
        t0 = time.perf_counter()
        fn()
        host[k] = (time.perf_counter() - t0) * 1e3
        assert s.sync()
    # the two routes give the same blocks
    legs["b_columns_of_32_pairs"]()
    assert s.sync()
    X = out[:n * d * len(distinct)].view(d * len(distinct), n).cpu().numpy().T
    legs["a_blocks_32_pairs"]()
    assert s.sync()
    B = blocks[:32 * d * d].cpu().numpy().reshape(32, d, d).transpose(0, 2, 1)
    where = {int(c): i for i, c in enumerate(distinct)}
    agree = max(float(np.abs(B[k] - X[d * r:d * r + d, d * where[int(c)]:d * where[int(c)] + d]).max() /
                      np.abs(B[k]).max()) for k, (r, c) in enumerate(zip(rows32, cols32)))
    ws = 8.0 * n * 48

    def leg(k, out_bytes):
        t = np.asarray(times[k])
        return {"ms_median": round(float(np.median(t)), 4), "ms_min": round(float(t.min()), 4), "ms_max": round(float(t.max()), 4),
                "host_enqueue_ms": round(host[k], 4), "device_bytes_workspace": ws, "device_bytes_output": out_bytes}
    return {
        "case": name + " pairs", "n_bcols": nb, "n_scalars": n, "dense_dim": plan["dense_dim"], "etree_height": st["etree_height"],
        "reps": reps, "repeats": repeats, "distinct_columns_of_32_pairs": int(len(distinct)),
        "a_blocks_32_pairs": leg("a_blocks_32_pairs", 8.0 * 32 * d * d),
        "b_columns_of_32_pairs": leg("b_columns_of_32_pairs", 8.0 * n * d * len(distinct)),
        "c_blocks_last_vs_64": leg("c_blocks_last_vs_64", 8.0 * 64 * d * d),
        "c_columns_last": leg("c_columns_last", 8.0 * n * d),
        "blocks_vs_columns_rel_inf": agree,
    }


def schur_pairs_case(name, lam, reps, repeats):
    dev = torch.device("cuda:0")
    s = CLinearSolver_Schur_HIP()
    s.SymbolicDecomposition_Blocky(lam)
    lib, h = s._lib, s._h
    n, nb, nc = lam.n_scalars, lam.n_bcols, lam.n_matrix_cut
    dims = np.diff(lam.cumsum).astype(np.int64)
    dc, dp = int(dims[0]), int(dims[nc])
    vals = torch.from_numpy(lam.values).to(dev)
    rng = np.random.default_rng(17)
    # 32 mixed pairs: 8 each of camera-camera, camera-landmark, landmark-camera, landmark-landmark
    cam, pt = (lambda k: rng.integers(0, nc, k)), (lambda k: rng.integers(nc, nb, k))
    rows32 = np.ascontiguousarray(np.concatenate([cam(8), cam(8), pt(8), pt(8)]), dtype=np.int64)
    cols32 = np.ascontiguousarray(np.concatenate([cam(8), pt(8), cam(8), pt(8)]), dtype=np.int64)
    shuffle = rng.permutation(32)
    rows32, cols32 = np.ascontiguousarray(rows32[shuffle]), np.ascontiguousarray(cols32[shuffle])
    distinct = np.unique(np.concatenate([rows32, cols32])).astype(np.int64)
    k_distinct = int(dims[distinct].sum())
    one_cam = np.array([nc // 2], dtype=np.int64)
    cand = np.ascontiguousarray(np.sort(rng.choice(np.arange(nc, nb), size=64, replace=False)), dtype=np.int64)
    cam64 = np.full(64, nc // 2, dtype=np.int64)
    blocks = torch.empty(64 * dc * dc, dtype=torch.float64, device=dev)
    out = torch.empty(n * k_distinct, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()

    def rc(x):
        assert x == 0, s._error()

    bytes_before = s.stats()["device_bytes"]
    s.set_option("profile", 1)                                            # (this call only: which route answers)
    rc(lib.slampp_hip_schur_marginal_blocks_device_async(h, vals.data_ptr(), 32, _ptr(rows32), _ptr(cols32), blocks.data_ptr()))
    assert s.sync()                                                       # W, C^-1 and the factor of S are in place from here on
    route = "dense inverse of S" if "marginals_inverse" in s.profile() else "forward substitutions on the sparse factor of S"
    s.set_option("profile", 0)
    bytes_blocks = s.stats()["device_bytes"]
    blocks_fn, cols_fn = lib.slampp_hip_schur_marginal_blocks_device_async, lib.slampp_hip_schur_marginal_columns_device_async
    legs = {
        "a_blocks_32_pairs": lambda: rc(blocks_fn(h, None, 32, _ptr(rows32), _ptr(cols32), blocks.data_ptr())),
        "b_columns_of_32_pairs": lambda: rc(cols_fn(h, None, len(distinct), _ptr(distinct), out.data_ptr())),
        "c_blocks_camera_vs_64": lambda: rc(blocks_fn(h, None, 64, _ptr(cam64), _ptr(cand), blocks.data_ptr())),
        "c_blocks_64_vs_camera": lambda: rc(blocks_fn(h, None, 64, _ptr(cand), _ptr(cam64), blocks.data_ptr())),
        "c_columns_camera": lambda: rc(cols_fn(h, None, 1, _ptr(one_cam), out.data_ptr())),
    }
    times = {k: [] for k in legs}
    for _ in range(repeats):                                              # the legs alternate: drift hits all of them alike
        for k, fn in legs.items():
            times[k].append(device_ms(s, fn, reps))
    bytes_columns = s.stats()["device_bytes"]
    host = {}
    for k, fn in legs.items():
        t0 = time.perf_counter()
        fn()
        host[k] = (time.perf_counter() - t0) * 1e3
        assert s.sync()
    # the two routes give the same blocks (against the scale that bounds a cross-covariance)
    legs["b_columns_of_32_pairs"]()
    assert s.sync()
    X = out[:n * k_distinct].view(k_distinct, n).cpu().numpy().T
    legs["a_blocks_32_pairs"]()
    assert s.sync()
    B = blocks.cpu().numpy()
    cs = lam.cumsum
    col_at = dict(zip((int(c) for c in distinct), np.concatenate([[0], np.cumsum(dims[distinct])])))

    def x_block(r, c):
        return X[cs[r]:cs[r + 1], col_at[int(c)]:col_at[int(c)] + int(dims[c])]
    agree, at = 0.0, 0
    for r, c in zip(rows32, cols32):
        dr, dcc = int(dims[r]), int(dims[c])
        blk = B[at:at + dr * dcc].reshape(dcc, dr).T
        at += dr * dcc
        bound = np.sqrt(np.abs(x_block(r, r)).max() * np.abs(x_block(c, c)).max())
        agree = max(agree, float(np.abs(blk - x_block(r, c)).max() / bound))

    def leg(k, out_bytes):
        t = np.asarray(times[k])
        return {"ms_median": round(float(np.median(t)), 4), "ms_min": round(float(t.min()), 4), "ms_max": round(float(t.max()), 4),
                "host_enqueue_ms": round(host[k], 4), "device_bytes_output": out_bytes}
    red = s.reduced_stats()
    a, b = float(np.median(times["a_blocks_32_pairs"])), float(np.median(times["b_columns_of_32_pairs"]))
    return {
        "case": name + " schur pairs", "n_cams": nc, "n_points": nb - nc, "n_scalars": n, "reduced_system_sparse_in_solves": red["n_bcols"] > 0,
        "covariance_route": route,
        "reps": reps, "repeats": repeats, "distinct_columns_of_32_pairs": int(len(distinct)), "scalar_columns_of_32_pairs": k_distinct,
        "a_blocks_32_pairs": leg("a_blocks_32_pairs", 8.0 * float((dims[rows32] * dims[cols32]).sum())),
        "b_columns_of_32_pairs": leg("b_columns_of_32_pairs", 8.0 * n * k_distinct),
        "c_blocks_camera_vs_64": leg("c_blocks_camera_vs_64", 8.0 * 64 * dc * dp),
        "c_blocks_64_vs_camera": leg("c_blocks_64_vs_camera", 8.0 * 64 * dc * dp),
        "c_columns_camera": leg("c_columns_camera", 8.0 * n * dc),
        "columns_over_blocks": round(b / a, 2),
        "handle_device_bytes": {"analyzed": bytes_before, "after_blocks": bytes_blocks, "after_columns": bytes_columns},
        "blocks_vs_columns_over_scale": agree,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="C3 or C2 (--schur-pairs: C4_venice or C4_band)")
    ap.add_argument("--pairs", action="store_true", help="blocks at arbitrary pairs next to whole columns (see above)")
    ap.add_argument("--schur-pairs", action="store_true", help="the same for BA systems in Schur mode (see above)")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_covariance: needs the GPU")
    results = []
    cases = [("C3", lambda: synth.pose_chain(n=100000)), ("C2", lambda: synth.sphere(50, 50))]
    if a.schur_pairs:
        cases = [("C4_venice", lambda: synth.ba(1000, 500_000, mode="venice", seed=777)),
                 ("C4_band", lambda: synth.ba(1000, 500_000, k=4, mode="band", seed=777))]
    for name, make in cases:
        if a.only and a.only != name:
            continue
        if a.schur_pairs:
            r = schur_pairs_case(name, make(), a.reps, a.repeats)
        else:
            r = pairs_case(name, make(), a.reps, a.repeats) if a.pairs else case(name, make(), a.reps)
        print(json.dumps(r))
        results.append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
