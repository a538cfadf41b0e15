"""Every job shape of the landmark-major Schur assembly (csrc/schur_tiles.hip: schur_run_kernel<DC, DP, NT, diag, prefix,
quad>, schur_tile_kernel<DC, DP, 64, NL>, schur_tile_reduce_kernel<DC>, and the contribution lists beside them) at the
smallest BA system that produces it.  A case names the option schur_tiles, the development knobs and what it expects the host
analysis to choose; the test proves from the analysis' own report (the "[schur report]" lines under SLAMPP_HIP_PLAN_TIMING)
that the launch ran with those jobs -- a case whose shape is not there fails --, and holds three right-hand sides, a re-solve
on the kept W and C^-1, an incremental update and an indefinite landmark of the case's route to the dense refined reference,
with the reduced system written densely and through the inner sparse solver's arrays.  schur_variant_cases.py holds the
systems, schur_variant_util.py the builder, references, the analysis' rules restated and the checks; DESIGN.md ("Which test
guards which branch of the Schur assembly") maps instantiation -> gate -> test id.  Run with -s to read the report lines."""
import numpy as np
import pytest

import schur_variant_util as U
from schur_variant_cases import CASES, case_dims

pytestmark = pytest.mark.gpu

_reports = {}                             # (case, dims) -> the parsed report of its analysis


def _id(v):
    return v if isinstance(v, str) else f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("sparse", [0, 1], ids=["dense_S", "sparse_S"])
@pytest.mark.parametrize("name,dims", case_dims(), ids=_id)
def test_job_shape(monkeypatch, capfd, name, dims, sparse):
    fx, rep, _ = U.run_case(monkeypatch, capfd, CASES, name, dims, sparse)
    _reports[(name, dims)] = rep


@pytest.mark.parametrize("dims", U.DIMS, ids=_id)
@pytest.mark.parametrize("name", ["prefix_mode1", "prefix_auto"])
def test_prefix_runs_and_classes_on_their_own_agree(monkeypatch, capfd, name, dims):
    """SLAMPP_HIP_DEV_NO_PREFIX_RUNS on the systems of the prefix cases: every class a run (or tile, or list) of its own, no
    landmark ends before its run's list -- within 1e-11 of the chains' result, and both within the bound of the reference."""
    fx = U.fixture(CASES, name, dims)
    with_chains, rep = U.analyzed(monkeypatch, capfd, fx, 0)
    assert rep["routes"]["prefix"] == fx.design.route_counts()["prefix"] > 0
    monkeypatch.setenv("SLAMPP_HIP_DEV_NO_PREFIX_RUNS", "1")
    without, rep = U.analyzed(monkeypatch, capfd, fx, 0)
    assert rep["routes"]["prefix"] == 0 and not any(x for (_, _, x) in rep["runs"]), rep["lines"]
    a, b = fx.B[:, 0].copy(), fx.B[:, 0].copy()
    assert with_chains.Solve_PosDef_Blocky(fx.lam, a) and without.Solve_PosDef_Blocky(fx.lam, b)
    assert U.rel_inf(a, fx.X[:, 0]) < U.TOL and U.rel_inf(b, fx.X[:, 0]) < U.TOL
    assert U.rel_inf(b, a) < 1e-11


@pytest.mark.parametrize("dims", U.DIMS, ids=_id)
@pytest.mark.parametrize("name", ["all_routes_auto", "reduce_runs_and_tiles"])
def test_the_report_changes_no_bit(monkeypatch, capfd, name, dims):
    """The same solve with and without SLAMPP_HIP_PLAN_TIMING: the report is diagnostics only."""
    from slam_plus_plus_amd.hip_solver import CLinearSolver_Schur_HIP
    fx = U.fixture(CASES, name, dims)
    reported, rep = U.analyzed(monkeypatch, capfd, fx, 0)
    assert rep["routes"] is not None
    monkeypatch.delenv("SLAMPP_HIP_PLAN_TIMING", raising=False)
    silent = CLinearSolver_Schur_HIP(schur_tiles=fx.case.mode, schur_sparse=0)
    capfd.readouterr()
    assert silent.SymbolicDecomposition_Blocky(fx.lam)
    assert "[schur" not in capfd.readouterr().err
    a, b = fx.B[:, 0].copy(), fx.B[:, 0].copy()
    assert reported.Solve_PosDef_Blocky(fx.lam, a) and silent.Solve_PosDef_Blocky(fx.lam, b)
    assert np.array_equal(a, b) and U.rel_inf(a, fx.X[:, 0]) < U.TOL


@pytest.mark.parametrize("dims", U.DIMS, ids=_id)
def test_every_launch_of_the_enqueue_is_reached(monkeypatch, capfd, dims):
    """Over the cases of one block size: every (NT, diagonal, prefix) launch of tiles_enqueue_t has jobs in some case, with
    quads and one landmark a step -- but for the off-diagonal launches of one to three tiles a side, which Emit_Run() never
    fills: a job with cb < rb has a full column block, OB DC >= 60 lines, four tiles.  Every NL the block size has ran."""
    for name, d in case_dims():
        if d == dims and (name, d) not in _reports:      # (the cases test_job_shape has not run in this process are analyzed here)
            _reports[(name, d)] = U.analyzed(monkeypatch, capfd, U.fixture(CASES, name, d), 0)[1]
    launches, loads = set(), set()
    for (name, d), rep in _reports.items():
        if d != dims:
            continue
        for line in rep["lines"]:
            print(name, d, line)
        launches |= {key + (rec["quad"],) for key, rec in rep["runs"].items()}
        if rep["tiles"]:
            loads.add(rep["tiles"]["NL"])
    want = {(nt, 1, x, q) for nt in (1, 2, 3, 4) for x in (0, 1) for q in (0, 1)} | {(4, 0, x, 0) for x in (0, 1)}
    assert launches == want, (sorted(want - launches), sorted(launches - want))
    assert not any(d == 0 and nt < 4 for nt, d, _, _ in launches)
    assert loads == {6: {1, 2, 3}, 7: {1, 2, 3, 4}, 3: {1}}[dims[0]]
