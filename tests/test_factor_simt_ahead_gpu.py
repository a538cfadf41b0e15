"""The fetch-ahead form of the lane-per-task factor kernel (csrc/simt_factor_ahead.hip: factor_simt_kernel_ahead; knob
SLAMPP_HIP_DEV_SIMT_FACTOR_AHEAD): what column ci + 1 reads of Lambda and b -- the diagonal block, b_j and the first
SIMT_FACTOR_AHEAD blocks below the diagonal -- is requested into a register set while column ci is factored.  The operations and
their order are those of factor_simt_kernel, so the results of one handle with the knob at 0, at 1 and unset are required to be
bit-identical (np.array_equal, no tolerance), and each within variant_util.TOL of the case's reference: for a factor_solve, for a
second right-hand side on the kept factor, for a batch of three members and for the factor itself.  The launch lines of
SLAMPP_HIP_STAGE_TIMING say which form every launch took (unset, the knob leaves the form to paired launches that fit the chip in
one round), the stage lines of SLAMPP_HIP_PLAN_TIMING what the column loops of the cases meet."""
import re

import numpy as np
import pytest

import variant_util as V

pytestmark = pytest.mark.gpu

KNOB = "SLAMPP_HIP_DEV_SIMT_FACTOR_AHEAD"
LANES = {"simt": 1, "simt_backward": 1}   # the leaf stage by the lane-per-task kernels, forward and backward
TALL = {"subtree_size": 8, "leaf_size": 1, "dense_top_nb": 0}   # leaf tasks of up to eight columns (PLAN_OPTIONS: four)


def islands(n=400, d=6, seed=97):
    """A pose chain with loop closures and, disconnected from it, 40 single poses, 40 pairs and 40 paths of three, each
    component held by a prior of its own: leaf tasks of one, two and three columns, and last columns with no block below the
    diagonal.  (The system of tests/test_backward_simt_ahead_gpu.py.)"""
    from slam_plus_plus_amd import synth
    rng = np.random.default_rng(seed)
    ci = np.arange(n - 1)
    ends = np.arange(50, n, 50)
    ei, ej, first = [ci, ends - rng.integers(26, 51, size=len(ends))], [ci + 1, ends], []
    nv = n
    for size in (1, 2, 3):
        for _ in range(40):
            first.append(nv)
            ei.append(np.arange(nv, nv + size - 1))
            ej.append(np.arange(nv + 1, nv + size))
            nv += size
    lam = synth._assemble_pose_graph(nv, d, np.concatenate(ei).astype(np.int64), np.concatenate(ej).astype(np.int64), rng, 0.02, 100.0,
                                     f"islands_n{n}")
    off = lam.block_value_offsets()
    for j in first:                                        # (pose 0 has its prior already)
        k = int(lam.bcol_ptr[j + 1] - 1)
        lam.values[off[k]:off[k + 1]].reshape(d, d)[...] += 100.0 * np.eye(d)
    return lam


class Local:
    """A system of this file with its refined reference, as far as the checks below need variant_util.System."""

    def __init__(self, lam):
        self.lam, self.x_ref, self.d = lam, V.refined_solution(lam), int(lam.cumsum[1] - lam.cumsum[0])
        self._factors = {}

    factor_reference = V.System.factor_reference


_local = {}


def system(name):
    if name in V.SYSTEMS:
        return V.system(name)
    if name not in _local:
        _local[name] = Local({"islands": islands}[name]())
    return _local[name]


# name -> (system, options on top of the lane-per-task ones)
CASES = {
    "chain_short": ("chain6", V.PLAN_OPTIONS),
    "chain_tall": ("chain6", TALL),
    "hub_short": ("hub", V.PLAN_OPTIONS),
    "hub_tall": ("hub", TALL),
    "islands": ("islands", TALL),
}

_reached = {}                             # case -> parse_report() of its analysis


def parse_report(err):
    """The line Report_Simt_Factor (sparse_setup.hip) prints per lane-per-task stage under SLAMPP_HIP_PLAN_TIMING."""
    stages = {}
    for m in re.finditer(r"\[setup\] stage (\d+) factor lanes: (\d+) tasks in (\d+) chunks of width (\d+), (\d+) chunks with spare lanes, "
                         r"fetch ahead holds (\d+) blocks, one round holds (\d+) waves; tasks by columns:((?: \d+:\d+)*); "
                         r"columns by sub-diagonal blocks:((?: \d+:\d+)*); columns by sub-diagonal blocks with a source in Lambda:((?: \d+:\d+)*); "
                         r"columns by fill-in blocks:((?: \d+:\d+)*); fill-in blocks among the blocks held: (\d+)", err):
        hist = [{int(k): int(v) for k, v in (e.split(":") for e in g.split())} for g in m.groups()[7:11]]
        tasks, chunks, width, spare, ahead, waves = map(int, m.groups()[1:7])
        stages[int(m.group(1))] = {"tasks": tasks, "chunks": chunks, "width": width, "spare": spare, "ahead": ahead, "waves": waves,
                                   "by_cols": hist[0], "by_blocks": hist[1], "by_sources": hist[2], "by_fill": hist[3],
                                   "held_fill": int(m.group(12))}
        assert sum(hist[0].values()) == tasks
        assert sum(hist[1].values()) == sum(hist[2].values()) == sum(hist[3].values())
    return stages


def parse_launches(err):
    """What launch_factor_simt says per launch under SLAMPP_HIP_STAGE_TIMING: [(chunks, width, block size, members, LPT, fetch ahead)]."""
    return [(int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5)), m.group(6) == "fetch ahead")
            for m in re.finditer(r"stage_timing lane-per-task factor launch: (\d+) chunks, width (\d+), block size (\d+), (\d+) members, "
                                 r"LPT (\d+), (fetch ahead|fetch by column)", err)]


def analyzed(monkeypatch, capfd, case, **more):
    from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP
    name, options = CASES[case]
    monkeypatch.setenv("SLAMPP_HIP_DEV", "1")
    monkeypatch.setenv("SLAMPP_HIP_PLAN_TIMING", "1")
    monkeypatch.setenv("SLAMPP_HIP_STAGE_TIMING", "1")     # (read at analysis: the launches then say which form they take)
    sysrec = system(name)
    solver = CLinearSolver_HIP(**dict(options, **LANES, **more))
    capfd.readouterr()
    assert solver.SymbolicDecomposition_Blocky(sysrec.lam)
    report = parse_report(capfd.readouterr().err)
    monkeypatch.delenv("SLAMPP_HIP_PLAN_TIMING")
    if not more:
        _reached[case] = report
        assert 0 in report, "the leaf stage has no lane-per-task chunks"
    assert sysrec.d == 6
    return sysrec, solver


def batch(solver, lam, x_ref, K):
    """K members with the values of Lambda and the right-hand sides (k + 1) eta, even strides: one pass of launches."""
    import torch
    sv, sr = lam.values.shape[0] + 6, lam.n_scalars + 6
    sv, sr = sv + sv % 2, sr + sr % 2
    vals = torch.zeros(K * sv, dtype=torch.float64, device="cuda")
    rhs = torch.zeros(K * sr, dtype=torch.float64, device="cuda")
    v, r = torch.from_numpy(lam.values).cuda(), torch.from_numpy(lam.rhs).cuda()
    for k in range(K):
        vals[k * sv:k * sv + lam.values.shape[0]] = v
        rhs[k * sr:k * sr + lam.n_scalars] = (k + 1.0) * r
    torch.cuda.synchronize()
    assert vals.data_ptr() % 16 == 0 and rhs.data_ptr() % 16 == 0
    solver.factor_solve_batch_device_async(K, vals.data_ptr(), sv, rhs.data_ptr(), sr)
    assert solver.sync_batch(K) == [True] * K
    x = rhs.cpu().numpy()
    for k in range(K):
        assert V.rel_inf(x[k * sr:k * sr + lam.n_scalars], (k + 1.0) * x_ref) < V.TOL, k
    return x


def set_knob(monkeypatch, value):
    if value is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, str(value))


def check_launches(launches, value, stage, members):
    """Every lane-per-task factor launch took the form the knob asks for: 0 = by column, 1 = ahead, unset = ahead where the
    launch fits one round of the fetch-ahead form (the stage's waves, asked at analysis).  Two lanes a task at these sizes."""
    assert launches
    for chunks, width, d, n_members, lpt, ahead in launches:
        assert (chunks, width, d, n_members, lpt) == (stage["chunks"], stage["width"], 6, members, 2), launches
        want = {0: False, 1: True, None: chunks * members <= stage["waves"]}[value]
        assert ahead == want, (value, launches, stage)


@pytest.mark.parametrize("case", sorted(CASES))
def test_bit_equal_to_the_fetch_by_column(monkeypatch, capfd, case):
    sysrec, solver = analyzed(monkeypatch, capfd, case)
    lam, x_ref, stage = sysrec.lam, sysrec.x_ref, _reached[case][0]
    assert stage["waves"] > 0 and stage["chunks"] * 3 <= stage["waves"]    # (the small launches below are small by the rule)
    # (the first kept-factor solve of a handle switches the storing of inv(L_jj) on -- the other instantiation of either
    # kernel -- for every factorization after it: one round before the comparison puts every value of the knob on the same
    # footing, and the factorizations compared all store the inverses; the round itself runs the instantiation that does not)
    for value in (0, 1):
        set_knob(monkeypatch, value)
        solver_first = analyzed(monkeypatch, capfd, case)[1] if value else solver
        capfd.readouterr()
        eta = lam.rhs.copy()
        assert solver_first.Solve_PosDef_Blocky(lam, eta) and V.rel_inf(eta, x_ref) < V.TOL
        check_launches(parse_launches(capfd.readouterr().err), value, stage, 1)
        if value == 0:
            eta_first = eta
        else:
            assert np.array_equal(eta_first, eta)          # (no inverses stored: knob 0 on one handle, 1 on a fresh one)
    eta = lam.rhs.copy()
    assert solver.Solve_Again(eta)
    got = {}
    for value in (0, 1, None):
        set_knob(monkeypatch, value)
        capfd.readouterr()
        eta = lam.rhs.copy()
        assert solver.Solve_PosDef_Blocky(lam, eta) and V.rel_inf(eta, x_ref) < V.TOL
        check_launches(parse_launches(capfd.readouterr().err), value, stage, 1)
        again = -2.0 * lam.rhs                              # a second right-hand side on the kept factor
        assert solver.Solve_Again(again) and V.rel_inf(again, -2.0 * x_ref) < V.TOL
        capfd.readouterr()
        x_batch = batch(solver, lam, x_ref, 3)              # the member strides
        check_launches(parse_launches(capfd.readouterr().err), value, stage, 3)
        ok, st, l_values = solver.factorize(lam)            # the factor itself
        assert ok
        check_launches(parse_launches(capfd.readouterr().err), value, stage, 1)
        V.check_factor(sysrec, st, l_values)
        got[value] = (eta, again, x_batch, l_values)
    for value in (1, None):
        for x0, x1 in zip(got[0], got[value]):
            assert np.array_equal(x0, x1)


@pytest.mark.parametrize("case", ["chain_short", "hub_tall"])
def test_the_factor_in_the_natural_order_is_the_same_bits(monkeypatch, capfd, case):
    """The hand-back Factorize_PosDef_Blocky uses: the factor in the caller's order, whatever kernels that plan takes."""
    sysrec, solver = analyzed(monkeypatch, capfd, case, natural_order=1)
    got = {}
    for value in (0, 1):
        set_knob(monkeypatch, value)
        ok, st, l_values = solver.factorize(sysrec.lam)
        assert ok and np.array_equal(st["perm"], np.arange(sysrec.lam.n_bcols))
        V.check_factor(sysrec, st, l_values)
        got[value] = l_values
    assert np.array_equal(got[0], got[1])


def test_a_batch_beyond_one_round_keeps_the_fetch_by_column(monkeypatch, capfd):
    """Unset, the knob leaves a launch of more waves than one round of the fetch-ahead form holds to factor_simt_kernel; at 1
    the same batch takes the fetch-ahead form and gives the same bits."""
    sysrec, solver = analyzed(monkeypatch, capfd, "chain_short")
    lam, x_ref, stage = sysrec.lam, sysrec.x_ref, _reached["chain_short"][0]
    K = stage["waves"] // stage["chunks"] + 1
    assert stage["waves"] > 0 and stage["chunks"] * K > stage["waves"] and K <= 256, stage
    got = {}
    for value in (None, 1):
        set_knob(monkeypatch, value)
        capfd.readouterr()
        got[value] = batch(solver, lam, x_ref, K)
        check_launches(parse_launches(capfd.readouterr().err), value, stage, K)
    assert np.array_equal(got[None], got[1])


def test_an_indefinite_leaf_column_is_reported(monkeypatch, capfd):
    import torch
    sysrec, solver = analyzed(monkeypatch, capfd, "chain_tall")
    lam, stage = sysrec.lam, _reached["chain_tall"][0]
    plan = solver.plan()
    cols = V.stage_columns(plan, 0)
    bad = V.with_bad_column(lam, int(plan["perm"][int(cols[len(cols) // 2])]))
    for values, want in ((bad.values, False), (lam.values, True)):
        vals = torch.from_numpy(values).cuda()
        for value in (0, 1):
            set_knob(monkeypatch, value)
            rhs = torch.from_numpy(lam.rhs).cuda()
            torch.cuda.synchronize()
            capfd.readouterr()
            solver.factor_solve_device_async(vals.data_ptr(), rhs.data_ptr())
            assert solver.sync() is want, (value, want)
            check_launches(parse_launches(capfd.readouterr().err), value, stage, 1)
    assert V.rel_inf(rhs.cpu().numpy(), sysrec.x_ref) < V.TOL   # (the flag is clean again, and so is the solution)


@pytest.mark.parametrize("name", ["chain3", "chain7"])
def test_odd_block_sizes_solve_on_the_kernel_they_take(monkeypatch, capfd, name):
    monkeypatch.setenv("SLAMPP_HIP_STAGE_TIMING", "1")
    r = V.run_variant(monkeypatch, name, LANES, {"SLAMPP_HIP_DEV": 1, KNOB: 1}, [])
    assert r.simt_stage_count() >= 1                      # (the leaf stage went to the lane-per-task kernels)
    launches = parse_launches(capfd.readouterr().err)
    assert launches and not any(ahead for *_, ahead in launches), launches


def test_the_cases_reach_the_column_loops_edges(monkeypatch, capfd):
    """Over the cases together: tasks of one column (no fetch but the prologue's), of two, of three and of eight; columns with no
    block below the diagonal (both of a set's half blocks are stand-ins), with exactly as many as a register set holds and with
    more (the loop inside the column); a fill-in block among the blocks a set holds (a stand-in for a block that exists); chunks
    with spare lanes -- read from the analysis of each case (the ones the equality tests have not run yet are analyzed here)."""
    for case in sorted(CASES):
        if case not in _reached:
            analyzed(monkeypatch, capfd, case)
    stages = [_reached[case][0] for case in sorted(CASES)]
    ahead = stages[0]["ahead"]
    assert ahead >= 1 and all(s["ahead"] == ahead for s in stages)
    for n_cols in (1, 2, 3, 8):
        assert any(s["by_cols"].get(n_cols, 0) > 0 for s in stages), (n_cols, stages)
    assert any(s["by_blocks"].get(0, 0) > 0 for s in stages), stages
    assert any(s["by_blocks"].get(ahead, 0) > 0 for s in stages), stages
    assert any(0 < b < ahead and n > 0 for s in stages for b, n in s["by_blocks"].items()) or ahead == 1, stages
    assert any(n > 0 for s in stages for b, n in s["by_blocks"].items() if b > ahead), stages
    assert any(n > 0 for s in stages for b, n in s["by_fill"].items() if b > 0), stages
    assert any(s["held_fill"] > 0 for s in stages), stages
    assert any(s["spare"] > 0 for s in stages)
