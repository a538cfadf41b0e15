#!/usr/bin/env python3
"""Generates tests/golden/landmark/{lm2d,lm3d,stereo}.npz: small graphs with landmarks or stereo cameras and explicit vertex
states, their landmark / stereo edges evaluated by the reference's own vertex and edge classes through
tests/landmark_golden_driver.cpp (built here with the include paths and archives of oracle/Makefile.ref, exactly as
tests/golden/make_linearize_golden.py builds its driver).  Run where the reference is present:

    python -c "import __graft_entry__ as g; g.build()" && python tests/golden/make_landmark_golden.py

Per fixture the fields of the linearize fixtures: the inputs (``state``, ``cumsum``, ``v0``, ``v1``, ``z``, ``sigma_inv``,
``params``, ``dx``) and, from the reference, ``J0``, ``J1`` (per edge rd x d, stored row-major [E, rd, d]), ``expectation``,
``err``, ``chi2``, ``state_plus``, ``state_minus``; vertex 0 of every edge is the pose or camera.  Besides: ``n_first_pose``
and ``n_poses`` (the block columns [n_first_pose, n_first_pose + n_poses) are poses or cameras), ``n_regular`` (the loops use
the first n_regular edges) and, for lm2d and lm3d, the pose-pose edge set of the same graph as inputs alone (``a_v0``, ``a_v1``,
``a_z``, ``a_sigma_inv``: EDGE_SE2 / EDGE_SE3, whose reference values the linearize fixtures hold).  Data only; no reference
source text is stored.

lm2d    30 SE(2) poses, then 12 landmarks.  Set A: the 29 odometry edges and 5 loop edges.  Set B: range-bearing edges, every
        landmark seen from 3 to 6 poses; the headings are the se2 fixture's (they wrap both ways), and at least 3 bearing
        differences z - h exceed pi before they are folded (asserted).  The last three edges of B are "close": their landmarks
        (the last three, each with two or more regular observations) lie at distance exactly 0, 5e-6 and 2e-5 from the
        observing pose -- on either side of the reference's range clamp at 1e-5, and on it.
lm3d    15 landmarks FIRST, then 25 SE(3) poses: every landmark edge has vertex 0 behind vertex 1 with d0 != d1.  Set A:
        pose-pose edges.  Set B: landmark edges.  The pose rotations begin with the se3 fixture's angles (0, 1e-9, 1e-5, 1e-3,
        ..., 3.5 above pi).
        Both trajectories run twice round a circle of radius 3 (the 3D one climbing), the landmarks stand inside and outside
        it, and loop edges tie the second lap to the first.  The gauge of these graphs is held by the tests' unary factor
        alone, on one pose; Lambda's smallest eigenvalue is the bending of the whole graph about that pose, the first edge's
        information over sum |p_i - p_0|^2, so a trajectory that runs 30 units away (as the linearize fixtures' do) has
        cond(Lambda) = 1.5e6 and its solve is good to 1e-10 at best -- the bound of the tests on dx.  Kept within 6 units it is
        over ten times smaller.
stereo  6 cameras on a ring and 40 points seen by 2 to 4 cameras each; per-camera intrinsics, radial coefficient and
        baselines in 0.1 .. 0.5, one baseline exactly 0.  Schur mode: n_matrix_cut = 6."""
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import header_util  # noqa: E402
import landmark_model as LMK  # noqa: E402  (used for the measurements only; the outputs are the reference's)
import linearize_model as M  # noqa: E402
import make_linearize_golden as G  # noqa: E402  (informations, the SE(3) angles)
import torch  # noqa: E402


def build_driver(td):
    v = header_util._makefile_vars()
    libs = v["REFLIBS"].split()
    assert all(os.path.isfile(a) for a in libs), "build the reference's archives first (build())"
    flags = ["-w"] + v["OPT"].split() + v["CDEFS"].split() + v["CHOLMOD_DEFS"].split() + v["INC"].split()
    exe = os.path.join(td, "landmark_golden_driver")
    subprocess.run(["g++"] + flags + [os.path.join(ROOT, "tests", "landmark_golden_driver.cpp"), "-o", exe] + libs + ["-lrt", "-lm"],
                   check=True)
    return exe


def chain_edges(first, n, loops):
    """Odometry over the block columns [first, first + n) and the given (from, to) loop edges, as offsets into them."""
    v0 = [first + i - 1 for i in range(1, n)] + [first + a for a, _ in loops]
    v1 = [first + i for i in range(1, n)] + [first + b for _, b in loops]
    return np.array(v0, np.int64), np.array(v1, np.int64)


def observations(rng, positions, landmarks, counts):
    """(pose, landmark) pairs: landmark l from counts[l] of the 8 poses nearest to it."""
    pairs = []
    for l, n_seen in enumerate(counts):
        for p in sorted(rng.choice(nearest_poses(positions, landmarks[l])[:8], size=n_seen, replace=False)):
            pairs.append((int(p), l))
    return pairs


def nearest_poses(positions, landmark):
    return sorted(range(len(positions)), key=lambda p: float(np.linalg.norm(positions[p] - landmark)))


def two_laps(n, rng, noise=0.1):
    """n positions twice round a circle of radius 3 about (3, 0): [n, 2]."""
    a = 4 * math.pi * np.arange(n) / n
    return np.stack([3 - 3 * np.cos(a), 3 * np.sin(a)], 1) + rng.normal(0, noise, (n, 2))


def ring_of_landmarks(n, rng):
    """n landmarks round the same centre, alternately outside (radius 5) and inside (1.5) the trajectory: [n, 2]."""
    a = 2 * math.pi * (np.arange(n) + 0.5) / n
    r = np.where(np.arange(n) % 2, 1.5, 5.0)
    return np.stack([3 + r * np.cos(a), r * np.sin(a)], 1) + rng.normal(0, 0.2, (n, 2))


def lm2d_case(rng):
    n_poses, n_lm = 30, 12
    i = np.arange(n_poses)
    heading = np.fmod(0.9 * i, 2 * math.pi)                       # the se2 fixture's: drops by 2 pi between neighbours
    heading[15:] = -np.fmod(0.7 * np.arange(15, n_poses), 2 * math.pi)   # and turns the other way
    poses = np.concatenate([two_laps(n_poses, rng), heading[:, None]], 1)
    lms = ring_of_landmarks(n_lm, rng)
    counts = [3 + l % 4 for l in range(n_lm)]
    counts[-1] = 4                                               # (the close edge below is one more: 3 to 6 in all)
    pairs = observations(rng, poses[:, :2], lms, counts)
    n_regular = len(pairs)
    # the close edges: each of the last three landmarks is moved to the given distance from the nearest pose that is more
    # than 1 away from every pose that sees it, and that pose then sees it too; what it was seen from before stays (its
    # regular observations, at ordinary ranges)
    close_distance = [0.0, 5e-6, 2e-5]
    for k in range(3):
        l = n_lm - 3 + k
        seen_from = [q for q, m in pairs if m == l]              # (a lap apart two poses nearly coincide: not one of those either)
        p = next(q for q in nearest_poses(poses[:, :2], lms[l]) if np.linalg.norm(poses[seen_from, :2] - poses[q, :2], axis=1).min() > 1)
        assert sum(1 for _, m in pairs if m == l) >= 2
        direction = np.array([math.cos(0.7 + k), math.sin(0.7 + k)])
        lms[l] = poses[p, :2] + close_distance[k] * direction
        if k == 0:
            assert np.array_equal(lms[l], poses[p, :2])
        pairs.append((p, l))
    v0 = np.array([p for p, _ in pairs], np.int64)
    v1 = np.array([n_poses + l for _, l in pairs], np.int64)
    x0, x1 = torch.from_numpy(poses[v0]), torch.from_numpy(lms[v1 - n_poses])
    h = LMK.lm2d_expectation(x0, x1).numpy()
    # noise of 0.25 and 0.15 rad (the information matrices state about 0.15): with residuals of that size the Gauss-Newton loop
    # of the tests still takes steps of 1e-4 in its fifth iteration.  With 0.05 it had converged to 1e-6 by the fourth, and
    # a step that small comes from an eta whose terms have cancelled to their last digits: it cannot be held to a relative 1e-10
    z = h + np.stack([rng.normal(0, 0.25, len(v0)), rng.normal(0, 0.15, len(v0))], 1)
    z[:, 1] = np.arctan2(np.sin(z[:, 1]), np.cos(z[:, 1]))       # measured bearings in (-pi, pi]: z - h is off by a turn where h wrapped
    a_v0, a_v1 = chain_edges(0, n_poses, [(0, 15), (3, 18), (7, 22), (25, 10), (28, 13)])
    ha = M.se2_expectation(torch.from_numpy(poses[a_v0]), torch.from_numpy(poses[a_v1])).numpy()
    a_z = ha + rng.normal(0, 1, ha.shape) * [0.25, 0.25, 0.15]
    a_z[:, 2] = np.arctan2(np.sin(a_z[:, 2]), np.cos(a_z[:, 2]))
    cumsum = np.concatenate([3 * np.arange(n_poses), 3 * n_poses + 2 * np.arange(n_lm + 1)])
    return dict(state=np.concatenate([poses.ravel(), lms.ravel()]), cumsum=cumsum, v0=v0, v1=v1, z=z,
                sigma_inv=G.informations(rng, len(v0), 2), params=np.zeros(0), n_first_pose=0, n_poses=n_poses, n_regular=n_regular,
                a_v0=a_v0, a_v1=a_v1, a_z=a_z, a_sigma_inv=G.informations(rng, len(a_v0), 3))


def lm3d_case(rng):
    n_lm, n_poses = 15, 25
    angles = list(G.SE3_ANGLES[:11])                              # 0, 1e-9, 1e-5, 1e-3, ..., 2.7, 3.5
    total = 3.5
    while len(angles) < n_poses:
        total += 0.45
        angles.append(math.remainder(total, 2 * math.pi))
    i = np.arange(n_poses)
    axis = np.stack([1 + 0.15 * np.sin(0.3 * i), 0.4 + 0.15 * np.cos(0.2 * i), -0.3 + 0.1 * np.sin(0.5 * i)], 1)
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    rot = axis * np.array(angles)[:, None]
    t = np.concatenate([two_laps(n_poses, rng), (0.05 * i + rng.normal(0, 0.1, n_poses))[:, None]], 1)
    poses = np.concatenate([t, rot], 1)
    lms = np.concatenate([ring_of_landmarks(n_lm, rng), rng.normal(0.6, 0.5, (n_lm, 1))], 1)
    pairs = observations(rng, t, lms, [2 + l % 4 for l in range(n_lm)])
    for p in (0, 1, 2, 3, 10):                                   # every pose with one of the special rotations sees a landmark
        if p not in {q for q, _ in pairs}:
            pairs.append((p, int(np.argmin(np.linalg.norm(lms - t[p], axis=1)))))
    v0 = np.array([n_lm + p for p, _ in pairs], np.int64)
    v1 = np.array([l for _, l in pairs], np.int64)
    h = LMK.lm3d_expectation(torch.from_numpy(poses[v0 - n_lm]), torch.from_numpy(lms[v1])).numpy()
    z = h + rng.normal(0, 0.05, h.shape)
    a_v0, a_v1 = chain_edges(n_lm, n_poses, [(2, 14), (5, 17), (9, 21), (23, 11), (24, 12)])
    x0, x1 = torch.from_numpy(poses[a_v0 - n_lm]), torch.from_numpy(poses[a_v1 - n_lm])
    ha = M.se3_expectation(x0, x1)
    noise = torch.from_numpy(rng.normal(0, 0.05, ha.shape))
    a_z = torch.cat([ha[:, :3] + noise[:, :3], M.so3_log(M.so3_exp(ha[:, 3:]) @ M.so3_exp(noise[:, 3:]))], 1).numpy()
    limit = math.pi - 0.2                                         # (the rule of make_linearize_golden.py for SE(3) edges)
    assert np.linalg.norm(ha[:, 3:].numpy(), axis=1).max() < limit
    cumsum = np.concatenate([3 * np.arange(n_lm), 3 * n_lm + 6 * np.arange(n_poses + 1)])
    return dict(state=np.concatenate([lms.ravel(), poses.ravel()]), cumsum=cumsum, v0=v0, v1=v1, z=z,
                sigma_inv=G.informations(rng, len(v0), 3), params=np.zeros(0), n_first_pose=n_lm, n_poses=n_poses, n_regular=len(v0),
                a_v0=a_v0, a_v1=a_v1, a_z=a_z, a_sigma_inv=G.informations(rng, len(a_v0), 6))


def stereo_case(rng):
    n_cams, n_pts = 6, 40
    cams = np.empty((n_cams, 6))
    for c in range(n_cams):
        a = 2 * math.pi * c / n_cams
        C = np.array([8 * math.cos(a), 8 * math.sin(a), 1.5 * math.sin(3 * a) + 0.3])
        zc = -C / np.linalg.norm(C)
        xc = np.cross([0, 0, 1.0], zc)
        xc /= np.linalg.norm(xc)
        R = np.stack([xc, np.cross(zc, xc), zc])                 # world -> camera
        cams[c, :3] = -R @ C
        cams[c, 3:] = M.so3_log(torch.from_numpy(R)).numpy()
    pts = rng.normal(0, 1, (n_pts, 3)) * [1.5, 1.5, 1.0]
    baseline = np.array([0.1, 0.25, 0.0, 0.5, 0.33, 0.18])
    params = np.stack([500 + rng.uniform(-20, 20, n_cams), 500 + rng.uniform(-20, 20, n_cams), 320 + rng.uniform(-5, 5, n_cams),
                       240 + rng.uniform(-5, 5, n_cams), rng.uniform(-0.1, 0.1, n_cams), baseline], 1)
    v0, v1 = [], []
    for p in range(n_pts):
        for c in sorted(rng.choice(n_cams, size=2 + p % 3, replace=False)):
            v0.append(c), v1.append(n_cams + p)
    v0, v1 = np.array(v0, np.int64), np.array(v1, np.int64)
    K = torch.from_numpy(params[v0])
    z = LMK.stereo_expectation(torch.from_numpy(cams[v0]), torch.from_numpy(pts[v1 - n_cams]), K).numpy() + rng.normal(0, 0.5, (len(v0), 3))
    cams_est = cams + np.concatenate([rng.normal(0, 0.02, (n_cams, 3)), rng.normal(0, 0.005, (n_cams, 3))], 1)
    pts_est = pts + rng.normal(0, 0.03, pts.shape)
    cumsum = np.concatenate([6 * np.arange(n_cams), 6 * n_cams + 3 * np.arange(n_pts + 1)])
    return dict(state=np.concatenate([cams_est.ravel(), pts_est.ravel()]), cumsum=cumsum, v0=v0, v1=v1, z=z,
                sigma_inv=G.informations(rng, len(v0), 3) / 40, params=params.ravel(), n_first_pose=0, n_poses=n_cams, n_regular=len(v0))


def run_reference(exe, td, name, case, dx):
    d0, d1, rd = LMK.EDGE_SHAPES[name]
    n_edges = len(case["v0"])
    src, dst = os.path.join(td, name + ".in"), os.path.join(td, name + ".out")
    LMK.write_driver_input(src, name, dict(case, params=case["params"] if case["params"].size else None, dx=dx))
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
    out = np.fromfile(dst)
    n = len(case["state"])
    sizes = [n_edges * rd * d0, n_edges * rd * d1, n_edges * rd, n_edges * rd, 1, n, n]
    assert out.size == sum(sizes)
    J0, J1, h, err, chi2, plus, minus = np.split(out, np.cumsum(sizes)[:-1])
    return dict(J0=J0.reshape(n_edges, d0, rd).transpose(0, 2, 1).copy(), J1=J1.reshape(n_edges, d1, rd).transpose(0, 2, 1).copy(),
                expectation=h.reshape(n_edges, rd), err=err.reshape(n_edges, rd), chi2=np.float64(chi2[0]), state_plus=plus,
                state_minus=minus)


def main():
    with tempfile.TemporaryDirectory() as td:
        exe = build_driver(td)
        for name, make, seed in (("lm2d", lm2d_case, 41), ("lm3d", lm3d_case, 42), ("stereo", stereo_case, 43)):
            rng = np.random.default_rng(seed)
            case = make(rng)
            dx = rng.normal(0, 0.1, case["state"].shape) if name != "stereo" else rng.normal(0, 0.02, case["state"].shape)
            ref = run_reference(exe, td, name, case, dx)
            if name == "lm2d":
                wrapped = np.abs(case["z"][:, 1] - ref["expectation"][:, 1]) > math.pi
                assert wrapped.sum() >= 3, "fewer than 3 bearing differences wrap"
                seen = np.bincount(case["v1"] - case["n_poses"], minlength=12)
                assert seen.min() >= 3 and seen.max() <= 6, seen
                assert np.bincount(case["v1"][:case["n_regular"]] - case["n_poses"], minlength=12)[-3:].min() >= 2
                assert np.array_equal(ref["expectation"][-3:, 0] == 1e-5, [True, True, False]), ref["expectation"][-3:, 0]
            if name == "lm3d":
                assert (case["v0"] > case["v1"]).all()
                norms = np.linalg.norm(case["state"][45:].reshape(-1, 6)[:, 3:], axis=1)
                assert norms[0] == 0 and abs(norms[1] - 1e-9) < 1e-20 and abs(norms[2] - 1e-5) < 1e-16 and abs(norms[10] - 3.5) < 1e-12
            if name == "stereo":
                assert (case["params"].reshape(-1, 6)[:, 5] == 0).sum() == 1
            rec = dict(case)
            rec.update(ref, dx=dx)
            for k in ("n_first_pose", "n_poses", "n_regular"):
                rec[k] = np.int64(rec[k])
            os.makedirs(os.path.join(HERE, "landmark"), exist_ok=True)
            path = os.path.join(HERE, "landmark", f"{name}.npz")
            np.savez_compressed(path, **rec)
            print(f"landmark_{name}: verts={len(case['cumsum']) - 1} edges={len(case['v0'])} (+{len(case.get('a_v0', []))} pose-pose) "
                  f"flipped={int((case['v0'] > case['v1']).sum())} chi2={float(ref['chi2']):.6g} -> {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
