"""The two-wave form of the lane-per-task leaf backward kernel (csrc/simt_kernel.hip: backward_simt_kernel_branches; knob
SLAMPP_HIP_DEV_SIMT_BWD_BRANCHES): backward substitution runs a leaf task's tree from the top, so a workgroup of two waves runs
the join columns of a chunk of split tasks on wave 0 and, behind a barrier, the two bins of branch chains side by side; chunks
of whole tasks ride two to a workgroup.  Per column the operations and their order are those of backward_simt_ahead_kernel, so
the solutions of one handle with the knob at 0 and at 1 are required to be bit-identical (np.array_equal, no tolerance), and
each within variant_util.TOL of the case's reference: for Solve_PosDef_Blocky, for Solve_Again on the kept factor and for a
batch of three members, with the factor form's knob (SLAMPP_HIP_DEV_SIMT_FACTOR_BRANCHES) at 0 and at 1.  The handles are
analyzed with the knob at 1, where every shape with two bins splits: that is how systems of a few hundred block columns reach
the form.  Unset, launches of stages below 2 048 tasks keep the one-wave forms and their launch line.  The systems and options
are those of tests/test_factor_simt_ahead_gpu.py and the width-16 cases of tests/test_simt_branches_gpu.py."""
import re

import numpy as np
import pytest

import variant_util as V
import test_backward_simt_ahead_gpu as BA
import test_factor_simt_ahead_gpu as A
import test_simt_branches_gpu as B

pytestmark = pytest.mark.gpu

KNOB = "SLAMPP_HIP_DEV_SIMT_BWD_BRANCHES"
CASES = dict(A.CASES)
CASES.update({case: B.CASES[case] for case in ("chain_tall_w16", "islands_w16", "hub_short_w16")})

_reached = {}                             # case -> parse_report() of its analysis, stage 0


def parse_report(err):
    """The line Upload_Simt (sparse_setup.hip) prints per stage that has backward workgroup records under SLAMPP_HIP_PLAN_TIMING."""
    stages = {}
    for m in re.finditer(r"\[setup\] stage (\d+) backward branches: (\d+) split tasks in (\d+) split chunks, (\d+) whole chunks, "
                         r"(\d+) workgroups of two waves, width (\d+), T\* (\d+), longest chain (\d+), longest task (\d+); "
                         r"split tasks by \(longer bin, join columns\):((?: \(\d+,\d+\):\d+)*); split tasks with three tips or more: (\d+); "
                         r"segment columns with more than (\d+) blocks: (\d+); columns with two rows outside the task or more: (\d+); "
                         r"chunks with spare lanes: (\d+); LDS (\d+) bytes \(three table regions of (\d+) entries, two x regions of (\d+) doubles\), "
                         r"one round holds (\d+) workgroups", err):
        by = {(int(a), int(b)): int(n) for a, b, n in re.findall(r"\((\d+),(\d+)\):(\d+)", m.group(10))}
        names = ("split_tasks", "split", "whole", "groups", "width", "tstar", "chain", "longest", "tip3", "held", "long_cols", "two_outside",
                 "spare", "lds", "tab_region", "x_region", "round")
        g = [int(m.group(i)) for i in (2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 14, 15, 16, 17, 18, 19)]
        s = stages[int(m.group(1))] = dict(zip(names, g), by=by)
        assert sum(by.values()) == s["split_tasks"] and s["groups"] == s["split"] + (s["whole"] + 1) // 2
        assert s["lds"] == (3 * s["tab_region"] + 2 * s["x_region"]) * 8 <= 64 * 1024
        assert s["x_region"] == s["longest"] * 6 * s["width"]
    return stages


def parse_launches(err):
    """What launch_backward_simt says of a launch that takes the form: [(workgroups, split chunks, whole chunks, width, block size, members)]."""
    return [tuple(int(g) for g in m.groups())
            for m in re.finditer(r"stage_timing lane-per-task backward branches launch: (\d+) workgroups of two waves, (\d+) split chunks, "
                                 r"(\d+) whole chunks, width (\d+), block size (\d+), (\d+) members", err)]


def set_knob(monkeypatch, value, knob=KNOB):
    if value is None:
        monkeypatch.delenv(knob, raising=False)
    else:
        monkeypatch.setenv(knob, str(value))


def analyzed(monkeypatch, capfd, case, knob=1):
    """A handle of the case analyzed with the knob at `knob` (1: every two-bin shape splits; None: the rule)."""
    from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP
    name, options = CASES[case]
    monkeypatch.setenv("SLAMPP_HIP_DEV", "1")
    monkeypatch.setenv("SLAMPP_HIP_PLAN_TIMING", "1")
    monkeypatch.setenv("SLAMPP_HIP_STAGE_TIMING", "1")     # (read at analysis: the launches then say which form they take)
    set_knob(monkeypatch, knob)
    set_knob(monkeypatch, None, B.KNOB)
    sysrec = A.system(name)
    solver = CLinearSolver_HIP(**dict(options, **A.LANES))
    capfd.readouterr()
    assert solver.SymbolicDecomposition_Blocky(sysrec.lam)
    err = capfd.readouterr().err
    monkeypatch.delenv("SLAMPP_HIP_PLAN_TIMING")
    report, lanes = parse_report(err), BA.parse_report(err)
    assert 0 in lanes and sysrec.d == 6
    if knob == 1:
        assert 0 in report, "the leaf stage has no backward workgroup records"
        _reached[case] = report[0]
    return sysrec, solver, report, lanes


def check_launches(err, value, stage, lanes, members):
    """Every lane-per-task backward launch took the form asked for: True = the two-wave form with its own line, False = a
    one-wave form with the line it has always had (the fetch-ahead form at these sizes)."""
    new, old = parse_launches(err), BA.parse_launches(err)
    if value:
        assert new and not old, err
        for launch in new:
            assert launch == (stage["groups"], stage["split"], stage["whole"], lanes["width"], 6, members), (launch, stage)
    else:
        assert old and not new, err
        for chunks, width, d, n_members, ahead in old:
            assert (chunks, width, d, n_members) == (lanes["chunks"], lanes["width"], 6, members) and ahead, old


@pytest.mark.parametrize("case", sorted(CASES))
def test_bit_equal_to_the_one_wave_form(monkeypatch, capfd, case):
    sysrec, solver, report, lanes = analyzed(monkeypatch, capfd, case)
    lam, x_ref, stage, lanes = sysrec.lam, sysrec.x_ref, report[0], lanes[0]
    assert stage["split"] > 0 and stage["round"] > 0 and stage["groups"] * 3 <= stage["round"]
    assert stage["split"] + stage["whole"] == lanes["chunks"] and stage["width"] == lanes["width"]
    # (the first kept-factor solve of a handle switches the storing of inv(L_jj) on for every factorization after it -- other
    # instantiations of the factor kernels: one round before the comparison puts every setting below on the same footing, as in
    # tests/test_factor_simt_ahead_gpu.py; the round itself runs the new form on a factor without the inverses)
    set_knob(monkeypatch, 1)
    eta = lam.rhs.copy()
    assert solver.Solve_PosDef_Blocky(lam, eta) and V.rel_inf(eta, x_ref) < V.TOL
    assert solver.Solve_Again(eta)
    got = {}
    for factor_value in (0, 1):                             # (the factor's form changes no bit either: tests/test_simt_branches_gpu.py)
        set_knob(monkeypatch, factor_value, B.KNOB)
        for value in (0, 1):
            set_knob(monkeypatch, value)
            capfd.readouterr()
            eta = lam.rhs.copy()
            assert solver.Solve_PosDef_Blocky(lam, eta) and V.rel_inf(eta, x_ref) < V.TOL
            check_launches(capfd.readouterr().err, value, stage, lanes, 1)
            again = -2.0 * lam.rhs                          # a second right-hand side on the kept factor
            assert solver.Solve_Again(again) and V.rel_inf(again, -2.0 * x_ref) < V.TOL
            check_launches(capfd.readouterr().err, value, stage, lanes, 1)
            x_batch = A.batch(solver, lam, x_ref, 3)        # the member strides
            check_launches(capfd.readouterr().err, value, stage, lanes, 3)
            got[factor_value, value] = (eta, again, x_batch)
    for key in ((0, 1), (1, 0), (1, 1)):
        for x0, x1 in zip(got[0, 0], got[key]):
            assert np.array_equal(x0, x1), key


@pytest.mark.parametrize("knob_at_analysis", [1, None])
def test_unset_the_small_launches_keep_their_form_and_their_line(monkeypatch, capfd, knob_at_analysis):
    """Stages below 2 048 tasks are the lane kernels' only by option simt = 1: unset, the rule leaves them as they were, whether
    the handle has records of every two-bin shape (analyzed at 1) or those of the rule."""
    sysrec, solver, report, lanes = analyzed(monkeypatch, capfd, "chain_tall", knob=knob_at_analysis)
    assert lanes[0]["tasks"] < 2048
    set_knob(monkeypatch, None)
    capfd.readouterr()
    eta = sysrec.lam.rhs.copy()
    assert solver.Solve_PosDef_Blocky(sysrec.lam, eta) and V.rel_inf(eta, sysrec.x_ref) < V.TOL
    check_launches(capfd.readouterr().err, False, None, lanes[0], 1)


def test_the_cases_reach_every_kind_of_record(monkeypatch, capfd):
    """Over the cases together, read from the report lines of their analyses (the ones the equality tests have not run yet are
    analyzed here): a split task with one join column and one with two; a task of three tips (two chains in one bin); a segment
    column with more blocks than a register set holds (the fetch loop inside the column); a column with two rows outside the
    task; a chunk with spare lanes; an odd number of whole chunks (a workgroup whose second wave has no segment); widths 16, 32."""
    for case in sorted(CASES):
        if case not in _reached:
            analyzed(monkeypatch, capfd, case)
    stages = [_reached[case] for case in sorted(CASES)]
    assert {s["width"] for s in stages} == {16, 32}
    assert all(s["held"] == stages[0]["held"] >= 2 for s in stages)
    for joins in (1, 2):
        assert any(j == joins and n > 0 for s in stages for (b, j), n in s["by"].items()), (joins, stages)
    assert any(s["tip3"] > 0 for s in stages), stages
    assert any(s["long_cols"] > 0 for s in stages), stages
    assert any(s["two_outside"] > 0 for s in stages), stages
    assert any(s["spare"] > 0 for s in stages), stages
    assert any(s["whole"] % 2 == 1 for s in stages), stages
    assert any(s["whole"] >= 2 for s in stages), stages
    assert all(s["chain"] <= s["longest"] and s["tstar"] <= s["longest"] for s in stages), stages
