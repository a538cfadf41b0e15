"""Covariance blocks at arbitrary pairs of block columns (sparse mode): Marginal_Blocks / Joint_Marginal, that is
slampp_hip_marginal_blocks -- Lambda^-1(r, c) = Y_r^T Y_c from the pruned forward substitution alone -- against numpy's
inverse of the dense Lambda, at the project's covariance tolerance (tests/test_covariance_blocks_gpu.py), block by block:
every block's error is taken relative to that block's own largest entry."""
import functools

import numpy as np
import pytest

from slam_plus_plus_amd import synth
from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP, _ptr

pytestmark = pytest.mark.gpu
TOL = 1e-10
GOLDENS = ["chain6_n60", "chain3_n90", "chain7_n40", "sphere_8x8", "manhattan_n150"]
OPTION_SETS = ({"dense_top_nb": 0}, {"dense_top_nb": 2, "dense_top_min_dim": 0}, {})   # no / a forced / the default dense top


def rel_inf(x, ref):
    return float(np.abs(x - ref).max() / np.abs(ref).max())


def ref_block(lam, full, r, c):
    cs = lam.cumsum
    return full[cs[r]:cs[r + 1], cs[c]:cs[c + 1]]


def check_blocks(lam, full, pairs, blocks, what=""):
    """Every block against the inverse; returns the worst relative error (printed: pytest -s shows it)."""
    assert len(blocks) == len(pairs)
    worst = 0.0
    for (r, c), blk in zip(pairs, blocks):
        ref = ref_block(lam, full, r, c)
        assert blk.shape == ref.shape, (r, c)
        worst = max(worst, rel_inf(blk, ref))
    print(f"{lam.name if hasattr(lam, 'name') else ''} {what}: {len(pairs)} pairs, worst block rel_inf {worst:.2e}")
    assert worst < TOL, what
    return worst


@functools.lru_cache(maxsize=None)
def system(name):
    """(system, its dense inverse): computed once, shared by the tests, never written to."""
    if name == "sphere24":
        lam = synth.sphere(24, 24)
    elif name == "manhattan1200":
        lam = synth.manhattan(1200)
    elif name == "chain300":
        lam = synth.pose_chain(n=300, d=6, seed=3)
    else:
        from golden_util import load_golden
        lam = load_golden(name)[0]
    full = np.linalg.inv(lam.to_scipy().toarray())
    full.setflags(write=False)
    return lam, full


def block_cols(lam):
    return np.repeat(np.arange(lam.n_bcols), np.diff(lam.bcol_ptr))


def seeded_pairs(lam, seed, n_random=14, n_pattern=8, n_diag=5):
    """About 40 pairs: random ones (off the pattern for the most part) each with its transposed twin, stored blocks of
    Lambda, diagonal ones, one column against several (a repeated column), and one pair listed twice."""
    rng = np.random.default_rng(seed)
    n = lam.n_bcols
    pairs = []
    for _ in range(n_random):
        r, c = (int(x) for x in rng.choice(n, size=2, replace=False))
        pairs += [(min(r, c), max(r, c)), (max(r, c), min(r, c))]
    col = block_cols(lam)
    off = np.flatnonzero(lam.brow_idx != col)
    for k in rng.choice(off, size=min(n_pattern, off.size), replace=False):
        pairs.append((int(lam.brow_idx[k]), int(col[k])))
    pairs += [(int(c), int(c)) for c in rng.choice(n, size=n_diag, replace=False)]
    pairs += [(int(r), n - 1) for r in rng.choice(n - 1, size=4, replace=False)]
    pairs.append(pairs[0])
    order = rng.permutation(len(pairs))
    return [pairs[i] for i in order]


def check_transposes(pairs, blocks):
    at = {}
    for k, p in enumerate(pairs):
        at.setdefault(p, k)
    n_checked = 0
    for (r, c), k in at.items():
        if r > c and (c, r) in at:
            assert np.array_equal(blocks[k], blocks[at[(c, r)]].T), (r, c)
            n_checked += 1
    return n_checked


# ---- goldens ----

@pytest.mark.parametrize("name", GOLDENS)
def test_blocks_match_goldens(name):
    lam, full = system(name)
    pairs = seeded_pairs(lam, 11)
    assert len({x for p in pairs for x in p}) >= 12                    # more than one pass of 48 scalar columns
    in_pattern = set(zip(lam.brow_idx.tolist(), block_cols(lam).tolist()))
    assert any(p in in_pattern for p in pairs) and any(p not in in_pattern and p[::-1] not in in_pattern for p in pairs)
    for opts in OPTION_SETS:
        blocks = CLinearSolver_HIP(**opts).Marginal_Blocks(lam, pairs)
        check_blocks(lam, full, pairs, blocks, f"{name} {opts}")
        assert check_transposes(pairs, blocks) >= 10


# ---- dense top ----

@pytest.mark.parametrize("tiles", [0, 1])                              # the dense top factored densely / by its tile schedule
@pytest.mark.parametrize("name", ["sphere24", "manhattan1200"])
def test_blocks_with_dense_top(name, tiles):
    """Pairs with both columns in the dense top, one of them, and neither."""
    lam, full = system(name)
    solver = CLinearSolver_HIP(dense_top_tiles=tiles) if name == "sphere24" else \
        CLinearSolver_HIP(dense_top_nb=8, dense_top_min_dim=0, dense_top_tiles=tiles)
    solver.SymbolicDecomposition_Blocky(lam)
    plan = solver.plan()
    assert plan["dense_dim"] > 0
    top = plan["perm"][plan["dense_pos"] >= 0].astype(np.int64)       # the caller's columns in the dense top / below it
    below = plan["perm"][plan["dense_pos"] < 0].astype(np.int64)
    assert top.size >= 2 and below.size >= 2
    rng = np.random.default_rng(5)
    t, b = rng.choice(top, size=6, replace=False if top.size >= 6 else True), rng.choice(below, size=8, replace=False)
    pairs = [(int(t[i]), int(t[(i + 1) % 6])) for i in range(6)] + [(int(t[0]), int(t[0]))]          # both
    pairs += [(int(t[i]), int(b[i])) for i in range(4)] + [(int(b[i]), int(t[i + 2])) for i in range(4)]   # one
    pairs += [(int(b[i]), int(b[i + 1])) for i in range(7)] + [(int(b[3]), int(b[3]))]               # neither
    blocks = solver.Marginal_Blocks(lam, pairs)
    check_blocks(lam, full, pairs, blocks, f"{name} tiles={tiles}")


# ---- mixed block sizes ----

def mixed_system(seed, n_min=30, n_max=160):
    """A random positive definite system with block sizes 2 .. 8 (a chain plus chords)."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(n_min, n_max))
    dims = rng.choice([2, 3, 6, 7, 8], size=n)
    chords = int(rng.integers(n // 2, 2 * n))
    a, b = rng.integers(0, n, chords), rng.integers(0, n, chords)
    pairs = set(zip(range(n - 1), range(1, n))) | {(min(x, y), max(x, y)) for x, y in zip(a, b) if x != y}
    cs = np.concatenate([[0], np.cumsum(dims)]).astype(np.int64)
    M = np.zeros((cs[-1], cs[-1]))
    for r, c in pairs:
        B = 0.4 * rng.standard_normal((dims[r], dims[c]))
        M[cs[r]:cs[r + 1], cs[c]:cs[c + 1]] = B
        M[cs[c]:cs[c + 1], cs[r]:cs[r + 1]] = B.T
    M += np.eye(cs[-1]) * (np.abs(M).sum(axis=1).max() * 0.6 + 1.0)
    bcol_ptr, brow, vals = [0], [], []
    for c in range(n):
        for r in range(c + 1):
            if r == c or (r, c) in pairs:
                brow.append(r)
                vals.append(M[cs[r]:cs[r + 1], cs[c]:cs[c + 1]].T.ravel())
        bcol_ptr.append(len(brow))
    lam = synth.BlockSystem(cs, np.asarray(bcol_ptr, dtype=np.int64), np.asarray(brow, dtype=np.int32), np.concatenate(vals),
                            rng.standard_normal(int(cs[-1])), 0)
    return lam, M


@pytest.mark.parametrize("seed", range(4))
def test_blocks_mixed_block_sizes(seed):
    lam, M = mixed_system(900 + seed)
    full = np.linalg.inv(M)
    dims = np.diff(lam.cumsum)
    pairs = seeded_pairs(lam, seed, n_random=16)
    assert any(dims[r] < dims[c] for r, c in pairs) and any(dims[r] > dims[c] for r, c in pairs)   # rectangular, both ways
    solver = CLinearSolver_HIP(dense_top_nb=0)
    blocks = solver.Marginal_Blocks(lam, pairs)
    check_blocks(lam, full, pairs, blocks, f"mixed {seed}")
    assert check_transposes(pairs, blocks) >= 10
    # the flat output of the C entry, block by block: d_r x d_c column-major, one after the other in the listed order
    rows = np.ascontiguousarray([p[0] for p in pairs], dtype=np.int64)
    cols = np.ascontiguousarray([p[1] for p in pairs], dtype=np.int64)
    sizes = dims[rows] * dims[cols]
    flat = np.full(int(sizes.sum()) + 3, np.nan)                       # (three doubles beyond the end stay untouched)
    assert solver._check(solver._lib.slampp_hip_marginal_blocks(solver._h, None, len(pairs), _ptr(rows), _ptr(cols), _ptr(flat)))
    at = 0
    for k, (r, c) in enumerate(pairs):
        got = flat[at:at + sizes[k]]
        assert np.array_equal(got, blocks[k].T.ravel()), k             # column-major; the same call, the same bits
        assert rel_inf(got, ref_block(lam, full, r, c).T.ravel()) < TOL, k
        at += int(sizes[k])
    assert at == sizes.sum() and np.isnan(flat[at:]).all()


# ---- agreement with the other parts, on one handle ----

def test_agrees_with_the_other_parts():
    lam, full = system("chain300")
    n = lam.n_bcols
    solver = CLinearSolver_HIP()
    diag = solver.Marginals(lam)                                       # [n, 6, 6]
    picks = [0, 1, 57, 150, 298, 299]
    blocks = solver.Marginal_Blocks(lam, [(c, c) for c in picks], reuse_factor=True)
    for c, blk in zip(picks, blocks):
        assert rel_inf(blk, diag[c]) < TOL, c
    cov = solver.Marginals_Pattern(lam)
    col = block_cols(lam)
    off = np.flatnonzero(lam.brow_idx != col)
    ks = np.random.default_rng(2).choice(off, size=20, replace=False)
    blocks = solver.Marginal_Blocks(lam, [(int(lam.brow_idx[k]), int(col[k])) for k in ks], reuse_factor=True)
    for k, blk in zip(ks, blocks):
        assert rel_inf(blk, cov[36 * k:36 * k + 36].reshape(6, 6).T) < TOL, k
    c0 = 211
    X = solver.Marginal_Columns(lam, [c0], reuse_factor=True)
    blocks = solver.Marginal_Blocks(lam, [(r, c0) for r in range(n)], reuse_factor=True)
    for r, blk in enumerate(blocks):
        assert rel_inf(blk, X[6 * r:6 * r + 6]) < TOL, r
    check_blocks(lam, full, [(r, c0) for r in range(n)], blocks, "chain300 column")
    bcols = [299, 0, 57, 211, 3, 292, 150, 151, 12, 100]               # 60 scalar columns: more than one pass
    J = solver.Joint_Marginal(lam, bcols, reuse_factor=True)
    idx = np.concatenate([np.arange(6 * c, 6 * c + 6) for c in bcols])
    assert J.shape == (60, 60) and np.array_equal(J, J.T)
    assert rel_inf(J, full[np.ix_(idx, idx)]) < TOL
    for r, c in [(0, 1), (3, 7), (9, 0)]:
        assert rel_inf(J[6 * r:6 * r + 6, 6 * c:6 * c + 6], ref_block(lam, full, bcols[r], bcols[c])) < TOL
    for bad in ([], [3, 3], [1, 2, 1]):
        with pytest.raises(ValueError):
            solver.Joint_Marginal(lam, bad, reuse_factor=True)


# ---- stale workspace ----

@pytest.mark.parametrize("name", ["chain300", "sphere24"])            # without / with a dense top
def test_stale_workspace_rows_are_not_read(name):
    """The workspace keeps the rows of earlier passes and calls: a pair alone, and among 30 others, after a columns call
    and a large pairs call on the same handle, against a fresh handle's answer."""
    lam, full = system(name)
    n = lam.n_bcols
    rng = np.random.default_rng(9)
    pair = (n // 3, n - 5)
    fresh = CLinearSolver_HIP().Marginal_Blocks(lam, [pair])[0]
    assert rel_inf(fresh, ref_block(lam, full, *pair)) < TOL
    solver = CLinearSolver_HIP()
    solver.Marginal_Columns(lam, [n - 1, 0, n // 2, 7])
    many = [tuple(int(x) for x in rng.choice(n, size=2)) for _ in range(120)]
    solver.Marginal_Blocks(lam, many, reuse_factor=True)
    alone = solver.Marginal_Blocks(lam, [pair], reuse_factor=True)[0]
    others = [tuple(int(x) for x in rng.choice(n, size=2)) for _ in range(30)]
    listed = others[:17] + [pair] + others[17:]
    among = solver.Marginal_Blocks(lam, listed, reuse_factor=True)
    assert rel_inf(alone, fresh) < 1e-13 and rel_inf(among[17], fresh) < 1e-13
    check_blocks(lam, full, listed, among, f"{name} among others")
    again = solver.Marginal_Blocks(lam, listed, reuse_factor=True)
    assert all(np.array_equal(a, b) for a, b in zip(among, again))


# ---- the factor in place ----

@pytest.mark.parametrize("name", ["chain6_n60", "sphere_8x8"])
def test_factor_in_place(name):
    from golden_util import load_golden
    lam, ref = load_golden(name)
    pairs = seeded_pairs(lam, 4)
    fresh = CLinearSolver_HIP().Marginal_Blocks(lam, pairs)
    solver = CLinearSolver_HIP()
    solver.SymbolicDecomposition_Blocky(lam)
    with pytest.raises(ValueError):                                    # analyzed, no factor yet
        solver.Marginal_Blocks(lam, pairs, reuse_factor=True)
    eta = lam.rhs.copy()
    assert solver.Solve_PosDef_Blocky(lam, eta)
    reuse = solver.Marginal_Blocks(lam, pairs, reuse_factor=True)
    for a, b in zip(reuse, fresh):
        assert rel_inf(a, b) < 1e-13
    eta = lam.rhs.copy()
    assert solver.Solve_Again(eta) and rel_inf(eta, ref["x_cholmod_super"]) < TOL
    solver.Marginal_Blocks(lam, pairs)                                 # factors: the factor stays for another solve
    eta = lam.rhs.copy()
    assert solver.Solve_Again(eta) and rel_inf(eta, ref["x_cholmod_super"]) < TOL
    X = solver.Marginal_Columns(lam, [1], reuse_factor=True)           # ... and for the columns call
    assert rel_inf(X, system(name)[1][:, lam.cumsum[1]:lam.cumsum[2]]) < TOL


def test_not_positive_definite_leaves_no_factor():
    from golden_util import load_golden
    lam, _ = load_golden("indefinite_n40")
    solver = CLinearSolver_HIP()
    with pytest.raises(ArithmeticError):
        solver.Marginal_Blocks(lam, [(0, 5)])
    with pytest.raises(ValueError):
        solver.Marginal_Blocks(lam, [(0, 5)], reuse_factor=True)


# ---- refusals (every bad input is rejected on the host, before anything is enqueued) ----

def test_refusals():
    from slam_plus_plus_amd.hip_solver import CLinearSolver_Schur_HIP
    lam = synth.pose_chain(n=40, d=6, seed=2)
    solver = CLinearSolver_HIP()
    solver.SymbolicDecomposition_Blocky(lam)
    for bad in ([], [(-1, 3)], [(3, -1)], [(40, 3)], [(3, 40)], [(1, 2), (3, 40)]):
        with pytest.raises(ValueError):
            solver.Marginal_Blocks(lam, bad)
    rows, cols, out = np.array([1], dtype=np.int64), np.array([2], dtype=np.int64), np.empty(36)
    vals = np.ascontiguousarray(lam.values)
    for args in ((_ptr(vals), 1, None, _ptr(cols), _ptr(out)), (_ptr(vals), 1, _ptr(rows), None, _ptr(out)),
                 (_ptr(vals), 1, _ptr(rows), _ptr(cols), None), (_ptr(vals), 0, _ptr(rows), _ptr(cols), _ptr(out))):
        with pytest.raises(ValueError):
            solver._check(solver._lib.slampp_hip_marginal_blocks(solver._h, *args))
    ba = synth.ba(8, 200, seed=1)
    schur = CLinearSolver_Schur_HIP()
    schur.SymbolicDecomposition_Blocky(ba)
    with pytest.raises(NotImplementedError):                           # (the Schur class has no such method: the C entry refuses)
        schur._check(schur._lib.slampp_hip_marginal_blocks(schur._h, _ptr(np.ascontiguousarray(ba.values)), 1, _ptr(rows),
                                                           _ptr(cols), _ptr(np.empty(64))))
