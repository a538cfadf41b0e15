"""The two-wave form of the lane-per-task leaf factor kernel (csrc/simt_factor_ahead.hip: factor_simt_kernel_branches; knob
SLAMPP_HIP_DEV_SIMT_FACTOR_BRANCHES): a workgroup of two waves runs the two bins of branch chains of a chunk of split tasks side
by side and, behind a barrier, the join columns above them on wave 0; chunks of whole tasks ride two to a workgroup.  Per column
the operations and their order are those of factor_simt_kernel_ahead, so the results of one handle with the knob at 0 and at 1
are required to be bit-identical (np.array_equal, no tolerance), and each within variant_util.TOL of the case's reference: for a
factor_solve, for a second right-hand side on the kept factor, for a batch of three members and for the factor itself, in the
plan's order and in the natural order.  The handles are analyzed with the knob at 1, where every shape with two bins splits:
that is how systems of a few hundred block columns reach the form.  Unset, launches of stages below 2 048 tasks keep the
one-wave forms and their launch line.  The systems and options are those of tests/test_factor_simt_ahead_gpu.py."""
import re

import numpy as np
import pytest

import variant_util as V
import test_factor_simt_ahead_gpu as A

pytestmark = pytest.mark.gpu

KNOB = "SLAMPP_HIP_DEV_SIMT_FACTOR_BRANCHES"
NARROW = {"simt_width": 16}

# name -> (system, options on top of the lane-per-task ones)
CASES = dict(A.CASES)
CASES.update({"chain_tall_w16": ("chain6", dict(A.TALL, **NARROW)), "islands_w16": ("islands", dict(A.TALL, **NARROW)),
              "hub_short_w16": ("hub", dict(V.PLAN_OPTIONS, **NARROW))})

_reached = {}                             # case -> (parse_report() of its analysis, A.parse_report() of it)


def parse_report(err):
    """The line Upload_Simt (sparse_setup.hip) prints per stage that has workgroup records under SLAMPP_HIP_PLAN_TIMING."""
    stages = {}
    for m in re.finditer(r"\[setup\] stage (\d+) factor branches: (\d+) split tasks in (\d+) split chunks, (\d+) whole chunks, "
                         r"(\d+) workgroups of two waves, T\* (\d+), longest chain (\d+), longest task (\d+); "
                         r"split tasks by \(longer bin, join columns\):((?: \(\d+,\d+\):\d+)*); LDS (\d+) bytes, "
                         r"one round holds (\d+) workgroups", err):
        by = {(int(a), int(b)): int(n) for a, b, n in re.findall(r"\((\d+),(\d+)\):(\d+)", m.group(9))}
        g = [int(m.group(i)) for i in (2, 3, 4, 5, 6, 7, 8, 10, 11)]
        stages[int(m.group(1))] = dict(zip(("split_tasks", "split", "whole", "groups", "tstar", "chain", "longest", "lds", "round"), g), by=by)
        assert sum(by.values()) == g[0] and g[3] == g[1] + (g[2] + 1) // 2
    return stages


def parse_launches(err):
    """What launch_factor_simt says of a launch that takes the form: [(workgroups, split chunks, whole chunks, width, block size, members)]."""
    return [tuple(int(g) for g in m.groups())
            for m in re.finditer(r"stage_timing lane-per-task factor branches launch: (\d+) workgroups of two waves, (\d+) split chunks, "
                                 r"(\d+) whole chunks, width (\d+), block size (\d+), (\d+) members", err)]


def analyzed(monkeypatch, capfd, case, knob=1, **more):
    """A handle of the case analyzed with the knob at `knob` (1: every two-bin shape splits; None: the rule)."""
    from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP
    name, options = CASES[case]
    monkeypatch.setenv("SLAMPP_HIP_DEV", "1")
    monkeypatch.setenv("SLAMPP_HIP_PLAN_TIMING", "1")
    monkeypatch.setenv("SLAMPP_HIP_STAGE_TIMING", "1")
    set_knob(monkeypatch, knob)
    sysrec = A.system(name)
    solver = CLinearSolver_HIP(**dict(options, **A.LANES, **more))
    capfd.readouterr()
    assert solver.SymbolicDecomposition_Blocky(sysrec.lam)
    err = capfd.readouterr().err
    monkeypatch.delenv("SLAMPP_HIP_PLAN_TIMING")
    report, lanes = parse_report(err), A.parse_report(err)
    if knob == 1 and not more:
        _reached[case] = (report, lanes)
    assert 0 in lanes and sysrec.d == 6
    return sysrec, solver, report, lanes


def set_knob(monkeypatch, value):
    if value is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, str(value))


def check_launches(err, value, stage, lanes, members):
    """Every lane-per-task factor launch took the form asked for: True = the two-wave form with its own line, False = a
    one-wave form with the line it has always had."""
    new, old = parse_launches(err), A.parse_launches(err)
    if value:
        assert new and not old, err
        for launch in new:
            assert launch == (stage["groups"], stage["split"], stage["whole"], lanes["width"], 6, members), (launch, stage)
    else:
        assert old and not new, err
        for chunks, width, d, n_members, lpt, ahead in old:
            assert (chunks, width, d, n_members, lpt) == (lanes["chunks"], lanes["width"], 6, members, 2), old


@pytest.mark.parametrize("case", sorted(CASES))
def test_bit_equal_to_the_one_wave_form(monkeypatch, capfd, case):
    sysrec, solver, report, lanes = analyzed(monkeypatch, capfd, case)
    lam, x_ref, stage, lanes = sysrec.lam, sysrec.x_ref, report[0], lanes[0]
    assert stage["split"] > 0 and stage["round"] > 0 and stage["groups"] * 3 <= stage["round"]
    assert stage["split"] + stage["whole"] == lanes["chunks"]
    # (the first factorization of a handle does not store inv(L_jj), those after its first kept-factor solve do: the two
    # instantiations of either kernel.  First the one that does not: knob 0 on this handle, 1 on a fresh one)
    for value in (0, 1):
        solver_first = analyzed(monkeypatch, capfd, case)[1] if value else solver
        set_knob(monkeypatch, value)
        capfd.readouterr()
        eta = lam.rhs.copy()
        assert solver_first.Solve_PosDef_Blocky(lam, eta) and V.rel_inf(eta, x_ref) < V.TOL
        check_launches(capfd.readouterr().err, value, stage, lanes, 1)
        if value == 0:
            eta_first = eta
        else:
            assert np.array_equal(eta_first, eta)
    eta = lam.rhs.copy()
    assert solver.Solve_Again(eta)
    got = {}
    for value in (0, 1):
        set_knob(monkeypatch, value)
        capfd.readouterr()
        eta = lam.rhs.copy()
        assert solver.Solve_PosDef_Blocky(lam, eta) and V.rel_inf(eta, x_ref) < V.TOL
        check_launches(capfd.readouterr().err, value, stage, lanes, 1)
        again = -2.0 * lam.rhs                              # a second right-hand side on the kept factor
        assert solver.Solve_Again(again) and V.rel_inf(again, -2.0 * x_ref) < V.TOL
        capfd.readouterr()
        x_batch = A.batch(solver, lam, x_ref, 3)            # the member strides
        check_launches(capfd.readouterr().err, value, stage, lanes, 3)
        ok, st, l_values = solver.factorize(lam)            # the factor itself, in the plan's order
        assert ok
        check_launches(capfd.readouterr().err, value, stage, lanes, 1)
        V.check_factor(sysrec, st, l_values)
        got[value] = (eta, again, x_batch, l_values)
    for x0, x1 in zip(got[0], got[1]):
        assert np.array_equal(x0, x1)


@pytest.mark.parametrize("case", ["chain_short", "hub_tall"])
def test_the_factor_in_the_natural_order_is_the_same_bits(monkeypatch, capfd, case):
    sysrec, solver, report, lanes = analyzed(monkeypatch, capfd, case, natural_order=1)
    got = {}
    for value in (0, 1):
        set_knob(monkeypatch, value)
        capfd.readouterr()
        ok, st, l_values = solver.factorize(sysrec.lam)
        assert ok and np.array_equal(st["perm"], np.arange(sysrec.lam.n_bcols))
        check_launches(capfd.readouterr().err, value, report[0], lanes[0], 1)
        V.check_factor(sysrec, st, l_values)
        got[value] = l_values
    assert np.array_equal(got[0], got[1])


@pytest.mark.parametrize("knob_at_analysis", [1, None])
def test_unset_the_small_launches_keep_their_form_and_their_line(monkeypatch, capfd, knob_at_analysis):
    """Stages below 2 048 tasks are the lane kernels' only by option simt = 1: unset, the rule leaves them as they were, whether
    the handle has records of every two-bin shape (analyzed at 1) or those of the rule."""
    sysrec, solver, report, lanes = analyzed(monkeypatch, capfd, "chain_tall", knob=knob_at_analysis)
    assert lanes[0]["tasks"] < 2048
    if knob_at_analysis == 1:
        assert 0 in report
    set_knob(monkeypatch, None)
    capfd.readouterr()
    eta = sysrec.lam.rhs.copy()
    assert solver.Solve_PosDef_Blocky(sysrec.lam, eta) and V.rel_inf(eta, sysrec.x_ref) < V.TOL
    err = capfd.readouterr().err
    check_launches(err, False, None, lanes[0], 1)
    assert all(ahead for *_, ahead in A.parse_launches(err))   # (the fetch-ahead form, as before)


def test_a_batch_beyond_one_round_keeps_the_one_wave_forms(monkeypatch, capfd):
    """Unset, a launch of more workgroups than one round of the two-wave form holds keeps today's forms; at 1 the same batch
    takes the two-wave form and gives the same bits."""
    sysrec, solver, report, lanes = analyzed(monkeypatch, capfd, "chain_short")
    lam, x_ref, stage = sysrec.lam, sysrec.x_ref, report[0]
    K = stage["round"] // stage["groups"] + 1
    assert stage["round"] > 0 and stage["groups"] * K * 2 > stage["round"] * 2 and K <= 256, stage
    got = {}
    for value in (None, 1):
        set_knob(monkeypatch, value)
        capfd.readouterr()
        got[value] = A.batch(solver, lam, x_ref, K)
        check_launches(capfd.readouterr().err, value, stage, lanes[0], K)
    assert np.array_equal(got[None], got[1])


def task_segments(plan, t):
    """simt_task_segments() (csrc/sparse_records.cpp) of task t of the plan: the bins and the join columns, as columns of the plan."""
    cols = [int(c) for c in plan["task_cols"][plan["task_ptr"][t]:plan["task_ptr"][t + 1]]]
    n = len(cols)
    parent = []
    for i, j in enumerate(cols):
        rows = set(int(r) for r in plan["lrow"][plan["lptr"][j] + 1:plan["lptr"][j + 1]])
        parent.append(next((i2 for i2 in range(i + 1, n) if cols[i2] in rows), -1))
    children = [sum(1 for p in parent if p == i) for i in range(n)]
    join = [c >= 2 for c in children]
    for i in range(n):
        if join[i] and parent[i] >= 0:
            join[parent[i]] = True
    chains = []
    for i in range(n):
        if children[i] == 0:
            chain, c = [], i
            while c >= 0 and not join[c]:
                chain.append(c)
                c = parent[c]
            chains.append(chain)
    bins = [[], []]
    for chain in sorted(chains, key=lambda c: -len(c)):     # (stable: ties keep the tips' order)
        bins[1 if len(chains) > 1 and len(bins[1]) < len(bins[0]) else 0] += chain
    return [sorted(cols[i] for i in b) for b in bins] + [[cols[i] for i in range(n) if join[i]]]


@pytest.mark.parametrize("where", ["second_bin", "joins"])
def test_an_indefinite_pivot_is_reported_by_either_wave(monkeypatch, capfd, where):
    """The flag of a column that wave 1 factors, and of a join column behind the barrier; the next solve is clean."""
    import torch
    sysrec, solver, report, lanes = analyzed(monkeypatch, capfd, "chain_tall")
    lam, stage = sysrec.lam, report[0]
    plan = solver.plan()
    picked = None
    for t in range(int(plan["stage_ptr"][0]), int(plan["stage_ptr"][1])):
        bins0, bins1, joins = task_segments(plan, t)
        if bins1 and joins:
            picked = (bins1 if where == "second_bin" else joins)[-1]
            break
    assert picked is not None
    bad = V.with_bad_column(lam, int(plan["perm"][picked]))
    for values, want in ((bad.values, False), (lam.values, True)):
        vals = torch.from_numpy(values).cuda()
        for value in (0, 1):
            set_knob(monkeypatch, value)
            rhs = torch.from_numpy(lam.rhs).cuda()
            torch.cuda.synchronize()
            capfd.readouterr()
            solver.factor_solve_device_async(vals.data_ptr(), rhs.data_ptr())
            assert solver.sync() is want, (value, want)
            check_launches(capfd.readouterr().err, value, stage, lanes[0], 1)
    assert V.rel_inf(rhs.cpu().numpy(), sysrec.x_ref) < V.TOL   # (the flag is clean again, and so is the solution)


def test_the_cases_reach_every_kind_of_workgroup(monkeypatch, capfd):
    """Over the cases together, read from the report lines of their analyses and a launch line each: a chunk of split tasks, a
    pair of chunks of whole tasks, a single chunk of whole tasks, widths 16 and 32; join segments of two columns."""
    widths = set()
    for case in sorted(CASES):
        sysrec, solver, report, lanes = analyzed(monkeypatch, capfd, case)
        set_knob(monkeypatch, 1)
        capfd.readouterr()
        eta = sysrec.lam.rhs.copy()
        assert solver.Solve_PosDef_Blocky(sysrec.lam, eta) and V.rel_inf(eta, sysrec.x_ref) < V.TOL
        launches = parse_launches(capfd.readouterr().err)
        assert launches == [(report[0]["groups"], report[0]["split"], report[0]["whole"], lanes[0]["width"], 6, 1)], launches
        widths.add(launches[0][3])
    stages = [_reached[case][0][0] for case in sorted(CASES)]
    assert widths == {16, 32}
    assert any(s["split"] > 0 for s in stages), stages
    assert any(s["whole"] >= 2 for s in stages), stages
    assert any(s["whole"] % 2 == 1 for s in stages), stages
    assert any(j == 2 and n > 0 for s in stages for (b, j), n in s["by"].items()), stages
    assert all(s["chain"] <= s["longest"] and s["tstar"] <= s["longest"] for s in stages), stages
