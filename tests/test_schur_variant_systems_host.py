"""The fixtures of tests/test_schur_variants_gpu.py, checked on the CPU: every designed system is symmetric positive definite
with cond_2(Lambda) <= 1e6 (a condition on the inputs: the damping is chosen so that it holds), the CPU oracle's fp64 solution
is within 1e-12 (rel-inf) of the dense refined reference -- the reference stands two orders below the 1e-10 the device is held
to --, and the builder writes the layout synth.ba writes: synth.ba's systems rebuilt from their own camera lists give the same
structure arrays."""
import collections

import numpy as np
import pytest

import schur_variant_util as U
from schur_variant_cases import CASES, case_dims
from slam_plus_plus_amd import synth
from oracle import oracle_lib as O


def test_the_nt_buckets_are_those_of_the_tile_class():
    for dc, buckets in U.NT_BUCKETS.items():
        for nt, (first, last) in enumerate(buckets, start=1):
            assert {U.nt_of(dc, k) for k in range(first, last + 1)} == {nt}
        assert buckets[0][0] == 1 and buckets[-1][1] == U.ob_of(dc)
        assert all(b[0] == a[1] + 1 for a, b in zip(buckets, buckets[1:]))
        assert U.nt_of(dc, U.ob_of(dc) + 5) == 4            # beyond a block: the first job is a full block


@pytest.mark.parametrize("name,dims", case_dims(), ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_fixture_is_well_conditioned_and_the_oracle_agrees_with_the_reference(name, dims):
    fx = U.fixture(CASES, name, dims)
    lam, A = fx.lam, fx.A
    assert np.array_equal(A, A.T)
    w = np.linalg.eigvalsh(A)
    assert w[0] > 0 and w[-1] / w[0] <= U.COND_MAX, (w[0], w[-1])
    ok, x_oracle, _, _ = O.solve_schur(lam)
    assert ok
    err = U.rel_inf(x_oracle, fx.X[:, 0])
    assert err < U.ORACLE_TOL, err
    n_x = fx.n_x
    assert U.rel_inf(x_oracle[:n_x], fx.X[:n_x, 0]) < U.ORACLE_TOL and U.rel_inf(x_oracle[n_x:], fx.X[n_x:, 0]) < U.ORACLE_TOL
    # the reference solves what it was given: residuals of all four right-hand sides in long double
    ld = np.longdouble
    R = fx.B.astype(ld) - A.astype(ld) @ fx.X.astype(ld)
    assert float(np.abs(R).max() / np.abs(fx.B).max()) < 1e-13
    # the changed and the indefinite system the device tests use: the first solvable, the second refused by the oracle
    lam2, x2 = fx.changed
    ok, x2_oracle, _, _ = O.solve_schur(lam2)
    assert ok and U.rel_inf(x2_oracle, x2) < U.ORACLE_TOL
    assert O.solve_schur(U.with_indefinite_landmark(lam, fx.p_bad))[0] is False
    # every landmark is on the route its case says
    tags = collections.Counter(t[0] for t in fx.design.tags)
    assert sum(tags.values()) == lam.n_bcols - lam.n_matrix_cut and tags[fx.case.route] > 0


@pytest.mark.parametrize("seed", range(6))
def test_builder_writes_the_layout_of_synth_ba(seed):
    rng = np.random.default_rng(70 + seed)
    cam_dim, pt_dim = U.DIMS[seed % 3]
    mode = ["band", "uniform", "venice", "tracks"][seed % 4]
    lam = synth.ba(int(rng.integers(12, 46)), int(rng.integers(20, 300)), k=int(rng.integers(1, 7)), mode=mode, seed=seed,
                   cam_dim=cam_dim, pt_dim=pt_dim)
    again = U.build_system(U.camera_lists(lam), cam_dim, pt_dim, seed=seed, n_cams=lam.n_matrix_cut)
    for name in ("cumsum", "bcol_ptr", "brow_idx"):
        a, b = getattr(lam, name), getattr(again, name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    assert again.n_matrix_cut == lam.n_matrix_cut and again.values.shape == lam.values.shape and again.rhs.shape == lam.rhs.shape
    # ... and the values sit where the structure says: U_cp = Jc^T Jp of the dense matrix is what the blocks hold
    A = U.dense(again)
    assert np.array_equal(A, A.T) and np.linalg.eigvalsh(A)[0] > 0


def test_the_run_model_counts_jobs_as_the_analysis_does():
    """Emit_Run() restated: a run of 65 landmarks seen by 25 cameras at 6 x 6 -- three row blocks, pieces of 32."""
    jobs = U.run_jobs(6, [25] * 65)
    assert sum(jobs.values()) == 3 * 6                               # three pieces, six block pairs each
    assert jobs[(4, 1, 0, 32)] == 2 * 2 and jobs[(4, 0, 0, 32)] == 2 * 3 and jobs[(2, 1, 0, 32)] == 2   # last block: 5 cameras
    assert jobs[(4, 1, 0, 1)] == 2 and jobs[(4, 0, 0, 1)] == 3 and jobs[(2, 1, 0, 1)] == 1
    chain = U.run_jobs(6, [12, 12, 10, 10, 9])                      # two reach the second block; the first block's job masks
    assert chain == {(4, 1, 1, 5): 1, (4, 0, 0, 2): 1, (1, 1, 0, 2): 1}
    launches = U.launches_of(chain, {})
    assert launches[(4, 1, 1)]["quad"] == 1 and launches[(4, 0, 0)]["quad"] == 0 and launches[(1, 1, 0)]["quad"] == 1
