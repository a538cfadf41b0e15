"""Covariance blocks of BA systems at arbitrary pairs of block columns (Schur mode): Marginal_Blocks and Joint_Marginal of
CLinearSolver_Schur_HIP (slampp_hip_schur_marginal_blocks) against numpy's inverse of the dense Lambda, against the other
covariance calls of the class and against themselves (exact transposes, identical bits from call to call).

Tolerance: max|blk - ref| <= TOL * sqrt(max|Sigma_rr| max|Sigma_cc|), the scale that bounds a cross-covariance -- not the
block's own largest entry: on the band systems the blocks of far-apart pairs are 1e-46 of that scale, which the dense-inverse
route cannot resolve relative to themselves (and nobody needs it to).  The Gram formula in numpy stays at or under 6.2e-16 of
that scale on these generators (cond_2(Lambda) 6e2 to 2e3), so TOL = 1e-10 leaves the device five to six decades."""
import functools

import numpy as np
import pytest

from slam_plus_plus_amd import synth
from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP, CLinearSolver_Schur_HIP, _ptr
from test_schur_covariance_gpu import block_cols, system_from_dense

pytestmark = pytest.mark.gpu
TOL = 1e-10
DENSE, SPARSE, MARGINALS_DENSE = {"schur_sparse": 0}, {"schur_sparse": 1, "dense_top_nb": 0}, {"marginals_dense": 1}
# (an inner dense top: the reduced system's sparse inverse subset does not take one, so the covariances of such a handle
# come from the dense inverse of S -- the option set is accepted and answers, by the dense route)
INNER_TOP = {"schur_sparse": 1, "dense_top_nb": 2, "dense_top_min_dim": 0}
OPTION_SETS = {"dense": DENSE, "sparse": SPARSE, "marginals_dense": MARGINALS_DENSE, "inner_top": INNER_TOP}

SYSTEMS = {
    "band63": lambda: synth.ba(40, 400, k=4, mode="band", seed=1),
    "venice63": lambda: synth.ba(30, 300, mode="venice", seed=2),
    "uniform73": lambda: synth.ba(20, 200, k=4, mode="uniform", seed=3, cam_dim=7),
    "tracks32": lambda: synth.ba(40, 300, mode="tracks", seed=4, cam_dim=3, pt_dim=2),
    "band_sparse_S": lambda: synth.ba(200, 3000, k=4, mode="band", seed=3),
    "ba_12x150_venice": lambda: _golden("ba_12x150_venice"),
    "ba_10x120_band": lambda: _golden("ba_10x120_band"),
}
CASES = [(name, opt) for name in ("band63", "venice63", "uniform73", "tracks32") for opt in ("dense", "sparse", "marginals_dense")] + \
    [("band_sparse_S", "sparse"), ("band_sparse_S", "inner_top"), ("ba_12x150_venice", "dense"), ("ba_12x150_venice", "sparse"),
     ("ba_10x120_band", "dense"), ("ba_10x120_band", "sparse")]


def _golden(name):
    from golden_util import load_golden
    return load_golden(name)[0]


@functools.lru_cache(maxsize=None)
def system(name):
    """(lam, numpy's inverse of the dense Lambda, the seeded pair list): computed once, shared, never written to."""
    lam = SYSTEMS[name]()
    full = np.linalg.inv(lam.to_scipy().toarray())
    full.setflags(write=False)
    return lam, full, tuple(pair_list(lam))


def cams_of(lam, p):
    nc = lam.n_matrix_cut
    return set(int(r) for r in lam.brow_idx[lam.bcol_ptr[nc + p]:lam.bcol_ptr[nc + p + 1] - 1])


def pair_list(lam, seed=7):
    """About 40 pairs, shuffled: camera-camera, camera-landmark (observed and not), landmark-camera, landmark-landmark
    (sharing all, some or no cameras), each with its transposed twin; diagonals; one column against many; a pair listed
    twice; the longest track against the shortest."""
    rng = np.random.default_rng(seed)
    nc, n_pts = lam.n_matrix_cut, lam.n_bcols - lam.n_matrix_cut
    tracks = [cams_of(lam, p) for p in range(n_pts)]
    pairs = []
    for _ in range(3):
        a, b = rng.choice(nc, 2, replace=False)
        pairs.append((int(a), int(b)))
    for _ in range(2):
        q = int(rng.integers(n_pts))
        pairs.append((int(rng.choice(sorted(tracks[q]))), nc + q))                       # observed
        others = sorted(set(range(nc)) - tracks[q])
        if others:
            pairs.append((int(rng.choice(others)), nc + q))                              # not observed
        pairs.append((nc + int(rng.integers(n_pts)), int(rng.integers(nc))))             # landmark row, camera column
    p = int(rng.integers(n_pts))
    kinds = {"all": None, "some": None, "none": None}
    for q in rng.permutation(n_pts):
        if q == p:
            continue
        n_shared = len(tracks[p] & tracks[q])
        kind = "none" if n_shared == 0 else "all" if tracks[p] == tracks[q] else "some"
        if kinds[kind] is None:
            kinds[kind] = (nc + p, nc + int(q))
    pairs += [pq for pq in kinds.values() if pq is not None]
    pairs.append((nc + int(rng.integers(n_pts)), nc + int(rng.integers(n_pts))))
    pairs += [(c, r) for r, c in pairs]                                                  # the twins
    lengths = np.array([len(t) for t in tracks])
    pairs.append((nc + int(lengths.argmax()), nc + int(lengths.argmin())))
    for d in (0, nc - 1, nc, nc + p, lam.n_bcols - 1):                                   # diagonals
        pairs.append((d, d))
    pairs += [(1, nc + int(q)) for q in rng.choice(n_pts, 6, replace=False)]             # one column against many
    pairs.append(pairs[4])                                                               # listed twice
    return [pairs[i] for i in rng.permutation(len(pairs))]


def scale(lam, full, c):
    cs = lam.cumsum
    return float(np.abs(full[cs[c]:cs[c + 1], cs[c]:cs[c + 1]]).max())


def check_blocks(lam, full, pairs, blocks, what=""):
    cs = lam.cumsum
    assert len(blocks) == len(pairs)
    worst = 0.0
    for (r, c), blk in zip(pairs, blocks):
        ref = full[cs[r]:cs[r + 1], cs[c]:cs[c + 1]]
        assert blk.shape == ref.shape
        err = float(np.abs(blk - ref).max()) / np.sqrt(scale(lam, full, r) * scale(lam, full, c))
        worst = max(worst, err)
        assert err <= TOL, (what, r, c, err)
    return worst


@pytest.mark.parametrize("name,opt", CASES, ids=["%s-%s" % c for c in CASES])
def test_pairs_against_numpy(name, opt):
    lam, full, pairs = system(name)
    pairs = list(pairs)
    solver = CLinearSolver_Schur_HIP(**OPTION_SETS[opt])
    blocks = solver.Marginal_Blocks(lam, pairs)
    print(name, opt, "worst error / scale: %.2e" % check_blocks(lam, full, pairs, blocks))
    # a pair and its twin are exact transposes; a pair listed twice gives the same bits; a diagonal block is symmetric
    first = {}
    n_twins = 0
    for (r, c), blk in zip(pairs, blocks):
        if (r, c) in first:
            assert np.array_equal(blk, first[(r, c)])
        first[(r, c)] = blk
    for (r, c), blk in first.items():
        if (c, r) in first:
            n_twins += 1
            assert np.array_equal(blk, first[(c, r)].T), (r, c)
    assert n_twins >= 16
    # two calls on one handle, and a fresh handle: identical bits
    again = solver.Marginal_Blocks(lam, pairs)
    fresh = CLinearSolver_Schur_HIP(**OPTION_SETS[opt]).Marginal_Blocks(lam, pairs)
    for a, b, c in zip(blocks, again, fresh):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    if name == "band_sparse_S":                                                          # at least three passes of 48 columns
        dims = np.diff(lam.cumsum)
        assert sum(int(dims[c]) for c in set(c for pr in pairs for c in pr)) > 2 * 48


ROUTES = [("band63", "dense", False), ("band63", "sparse", True), ("band63", "marginals_dense", False),
          ("tracks32", "sparse", True), ("uniform73", "sparse", True), ("band_sparse_S", "sparse", True),
          ("band_sparse_S", "inner_top", False)]


@pytest.mark.parametrize("name,opt,b_sparse", ROUTES, ids=["%s-%s" % r[:2] for r in ROUTES])
def test_route_taken(name, opt, b_sparse):
    """Which route answers: the dense one inverts S (a "marginals_inverse" phase behind the factorization), the sparse one
    does not -- it runs forward substitutions on S's sparse factor, so the inner solver exists.  A silent fall from the sparse
    route to the dense inverse would leave every other test passing."""
    lam, full, pairs = system(name)
    solver = CLinearSolver_Schur_HIP(profile=1, **OPTION_SETS[opt])
    check_blocks(lam, full, list(pairs), solver.Marginal_Blocks(lam, list(pairs)))
    phases = solver.profile()
    assert phases.get("marginal_blocks", (0, 0.0))[0] == 1, phases
    assert phases.get("marginals_factor", (0, 0.0))[0] == 1, phases
    assert ("marginals_inverse" in phases) == (not b_sparse), phases
    if b_sparse or opt == "inner_top":
        assert solver.reduced_stats()["n_bcols"] == lam.n_matrix_cut
    elif opt == "dense":
        assert solver.reduced_stats()["n_bcols"] == 0


@pytest.mark.parametrize("opt", ["dense", "sparse", "marginals_dense"])
def test_consistent_with_the_other_covariance_calls(opt):
    lam, full, pairs = system("venice63")
    cs, nc, dims = lam.cumsum, lam.n_matrix_cut, np.diff(lam.cumsum)
    solver = CLinearSolver_Schur_HIP(**OPTION_SETS[opt])

    def close(blk, ref, r, c):
        return float(np.abs(blk - ref).max()) <= TOL * np.sqrt(scale(lam, full, r) * scale(lam, full, c))

    # the diagonal pairs are Schur_Marginals' blocks
    diag = [0, 7, nc - 1, nc, nc + 11, lam.n_bcols - 1]
    blocks = solver.Marginal_Blocks(lam, [(d, d) for d in diag])
    cams, pts = solver.Schur_Marginals(lam)
    for d, blk in zip(diag, blocks):
        assert close(blk, cams[d] if d < nc else pts[d - nc], d, d)
    # pairs inside Lambda's pattern are Marginals_Pattern's blocks
    cov = solver.Marginals_Pattern(lam)
    off, col = lam.block_value_offsets(), block_cols(lam)
    stored = np.random.default_rng(5).choice(len(col), 30, replace=False)
    stored_pairs = [(int(lam.brow_idx[i]), int(col[i])) for i in stored]
    blocks = solver.Marginal_Blocks(lam, stored_pairs, reuse_factor=True)
    for i, (r, c), blk in zip(stored, stored_pairs, blocks):
        assert close(blk, cov[off[i]:off[i + 1]].reshape(int(dims[c]), int(dims[r])).T, r, c)
    # the blocks are rows of Marginal_Columns for the same columns
    cols = [2, nc + 5, 9, nc + 40]
    X = solver.Marginal_Columns(lam, cols, reuse_factor=True)
    rows = [0, 2, nc + 5, nc + 77, 9, nc - 1]
    blocks = solver.Marginal_Blocks(lam, [(r, c) for c in cols for r in rows], reuse_factor=True)
    j0, k = 0, 0
    for c in cols:
        for r in rows:
            assert close(blocks[k], X[cs[r]:cs[r + 1], j0:j0 + int(dims[c])], r, c)
            k += 1
        j0 += int(dims[c])


@pytest.mark.parametrize("opt", ["dense", "sparse"])
def test_joint_marginal_of_a_mixed_set(opt):
    lam, full, _ = system("uniform73")
    cs, nc = lam.cumsum, lam.n_matrix_cut
    cols = [nc + 17, 3, nc + 100, 11, 0, nc + 4]                                         # three cameras, three landmarks
    joint = CLinearSolver_Schur_HIP(**OPTION_SETS[opt]).Joint_Marginal(lam, cols)
    idx = np.concatenate([np.arange(cs[c], cs[c + 1]) for c in cols])
    assert joint.shape == (len(idx), len(idx))
    assert np.array_equal(joint, joint.T)
    ref = full[np.ix_(idx, idx)]
    bound = np.sqrt(np.concatenate([np.full(int(cs[c + 1] - cs[c]), scale(lam, full, c)) for c in cols]))
    assert np.all(np.abs(joint - ref) <= TOL * np.outer(bound, bound))


@pytest.mark.parametrize("opt", ["dense", "sparse"])
def test_factor_reuse(opt):
    lam, full, pairs = system("band63")
    pairs = list(pairs)[:12]
    cs, nc = lam.cumsum, lam.n_matrix_cut
    solver = CLinearSolver_Schur_HIP(**OPTION_SETS[opt])
    with pytest.raises(ValueError):                                                      # nothing to reuse yet
        solver.Marginal_Blocks(lam, pairs, reuse_factor=True)
    cov = solver.Marginals_Pattern(lam)
    check_blocks(lam, full, pairs, solver.Marginal_Blocks(lam, pairs, reuse_factor=True), "after Marginals_Pattern")
    fresh = CLinearSolver_Schur_HIP(**OPTION_SETS[opt])
    check_blocks(lam, full, pairs, fresh.Marginal_Blocks(lam, pairs), "fresh")
    X = fresh.Marginal_Columns(lam, [nc + 3, 1], reuse_factor=True)
    ref = np.concatenate([full[:, cs[nc + 3]:cs[nc + 4]], full[:, cs[1]:cs[2]]], axis=1)
    assert np.abs(X - ref).max() < TOL * np.abs(ref).max()
    again = fresh.Marginals_Pattern(lam, reuse_factor=True)
    assert np.abs(again - cov).max() < TOL * np.abs(cov).max()
    check_blocks(lam, full, pairs, fresh.Marginal_Blocks(lam, pairs, reuse_factor=True), "after its own call")
    lam2 = synth.BlockSystem(lam.cumsum, lam.bcol_ptr, lam.brow_idx, lam.values * 2.0, lam.rhs, lam.n_matrix_cut)
    eta = lam2.rhs.copy()
    assert fresh.Solve_PosDef_Blocky(lam2, eta)                                          # an intervening solve on other values
    with pytest.raises(ValueError):
        fresh.Marginal_Blocks(lam, pairs, reuse_factor=True)


def test_not_positive_definite_leaves_nothing_to_reuse():
    from golden_util import load_golden
    lam, _ = load_golden("cond_ba_1e9_indefinite")
    solver = CLinearSolver_Schur_HIP()
    nc = lam.n_matrix_cut
    pairs = [(0, 1), (nc, 0), (nc + 1, nc + 1)]
    with pytest.raises(ArithmeticError):
        solver.Marginal_Blocks(lam, pairs)
    with pytest.raises(ValueError):
        solver.Marginal_Blocks(lam, pairs, reuse_factor=True)
    with pytest.raises(ValueError):
        solver.Marginal_Columns(lam, [0], reuse_factor=True)


def test_refusals():
    ba = synth.ba(8, 200, seed=1)
    vals = np.ascontiguousarray(ba.values)
    rows, cols = np.array([0, 9], dtype=np.int64), np.array([3, 1], dtype=np.int64)
    out = np.empty(2 * 36)

    def call(h, values, n_pairs, p_rows, p_cols, p_out):
        return h._check(h._lib.slampp_hip_schur_marginal_blocks(h._h, values, n_pairs, p_rows, p_cols, p_out))

    solver = CLinearSolver_Schur_HIP()
    solver.SymbolicDecomposition_Blocky(ba)
    with pytest.raises(ValueError):
        call(solver, _ptr(vals), 0, _ptr(rows), _ptr(cols), _ptr(out))
    with pytest.raises(ValueError):
        call(solver, _ptr(vals), 2, None, _ptr(cols), _ptr(out))
    with pytest.raises(ValueError):
        call(solver, _ptr(vals), 2, _ptr(rows), None, _ptr(out))
    with pytest.raises(ValueError):
        call(solver, _ptr(vals), 2, _ptr(rows), _ptr(cols), None)
    with pytest.raises(ValueError):                                                      # values = NULL: nothing to reuse
        call(solver, None, 2, _ptr(rows), _ptr(cols), _ptr(out))
    for bad in (-1, ba.n_bcols):
        for where in (rows, cols):
            spoiled = where.copy()
            spoiled[1] = bad
            with pytest.raises(ValueError):
                call(solver, _ptr(vals), 2, _ptr(spoiled) if where is rows else _ptr(rows),
                     _ptr(spoiled) if where is cols else _ptr(cols), _ptr(out))
    assert call(solver, _ptr(vals), 2, _ptr(rows), _ptr(cols), _ptr(out))               # the handle still answers
    sparse = CLinearSolver_HIP()                                                         # a sparse-mode handle
    sparse.SymbolicDecomposition_Blocky(ba)
    with pytest.raises(NotImplementedError):
        call(sparse, _ptr(vals), 2, _ptr(rows), _ptr(cols), _ptr(out))
    group = CLinearSolver_Schur_HIP(devices=[0, 0])
    group.SymbolicDecomposition_Blocky(ba)
    with pytest.raises(NotImplementedError):
        call(group, _ptr(vals), 2, _ptr(rows), _ptr(cols), _ptr(out))
    with pytest.raises(NotImplementedError):
        group.Marginal_Blocks(ba, [(0, 1)])


def test_fallback_answers_as_the_sparse_path():
    rng = np.random.default_rng(4)
    lam = synth.ba(12, 80, k=3, mode="uniform", seed=9)
    M = lam.to_scipy().toarray()
    nc, n_x = lam.n_matrix_cut, int(lam.cumsum[lam.n_matrix_cut])
    for p, q in ((3, 7), (10, 11)):                                                      # landmarks tied to each other: no Schur step
        a, b = n_x + 3 * p, n_x + 3 * q
        B = 0.05 * rng.standard_normal((3, 3))
        M[a:a + 3, b:b + 3] += B
        M[b:b + 3, a:a + 3] += B.T
    lam2 = system_from_dense(M, np.diff(lam.cumsum), lam.rhs, nc)
    pairs = [(0, 5), (nc + 3, 1), (nc + 7, nc + 3), (2, 2), (1, nc + 3), (nc + 10, nc + 11)]
    schur, sparse = CLinearSolver_Schur_HIP(), CLinearSolver_HIP()
    blocks, want = schur.Marginal_Blocks(lam2, pairs), sparse.Marginal_Blocks(lam2, pairs)
    full = np.linalg.inv(M)
    check_blocks(lam2, full, pairs, blocks)
    for a, b in zip(blocks, want):
        assert np.array_equal(a, b)
    for a, b in zip(schur.Marginal_Blocks(lam2, pairs, reuse_factor=True), blocks):
        assert np.array_equal(a, b)
    assert np.array_equal(schur.Joint_Marginal(lam2, [nc + 3, 1, nc + 7]), sparse.Joint_Marginal(lam2, [nc + 3, 1, nc + 7]))
