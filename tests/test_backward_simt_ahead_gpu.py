"""The fetch-ahead form of the lane-per-task backward kernel (csrc/simt_kernel.hip: backward_simt_ahead_kernel; knob
SLAMPP_HIP_DEV_SIMT_BWD_AHEAD): everything column ci - 1 reads from memory is requested into a second register set while column
ci is solved, a set holding the first SIMT_BWD_AHEAD blocks below the diagonal and x of one row outside the task.  The operations and their order are those of
backward_simt_kernel, so the solutions of one handle with the knob at 0 and at 1 are required to be bit-identical
(np.array_equal, no tolerance), and each within variant_util.TOL of the case's reference: for a factor_solve, for a second
right-hand side on the kept factor and for a batch of three members.  The launch lines of SLAMPP_HIP_STAGE_TIMING say which form
every launch took (unset, the knob leaves the form to launches that fit the chip in one round), the stage lines of
SLAMPP_HIP_PLAN_TIMING what the column loops of the cases meet."""
import re

import numpy as np
import pytest

import variant_util as V

pytestmark = pytest.mark.gpu

KNOB = "SLAMPP_HIP_DEV_SIMT_BWD_AHEAD"
LANES = {"simt": 1, "simt_backward": 1}   # the leaf stage by the lane-per-task kernels, forward and backward
TALL = {"subtree_size": 8, "leaf_size": 1, "dense_top_nb": 0}   # leaf tasks of up to eight columns (PLAN_OPTIONS: four)


def islands(n=400, d=6, seed=97):
    """A pose chain with loop closures and, disconnected from it, 40 single poses, 40 pairs and 40 paths of three, each
    component held by a prior of its own: leaf tasks of one, two and three columns, and last columns with no block below the
    diagonal."""
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
    """The line Report_Simt_Backward (sparse_setup.hip) prints per lane-per-task stage under SLAMPP_HIP_PLAN_TIMING."""
    stages = {}
    for m in re.finditer(r"\[setup\] stage (\d+) backward lanes: (\d+) tasks in (\d+) chunks of width (\d+), (\d+) chunks with spare lanes, "
                         r"fetch ahead holds (\d+) blocks, one round holds (\d+) waves; tasks by columns:((?: \d+:\d+)*); "
                         r"columns by sub-diagonal blocks:((?: \d+:\d+)*); columns by rows outside the task among the blocks held:((?: \d+:\d+)*); "
                         r"blocks with the row inside the task: (\d+), outside: (\d+)", err):
        hist = [{int(k): int(v) for k, v in (e.split(":") for e in g.split())} for g in m.groups()[7:10]]
        tasks, chunks, width, spare, ahead, waves = map(int, m.groups()[1:7])
        stages[int(m.group(1))] = {"tasks": tasks, "chunks": chunks, "width": width, "spare": spare, "ahead": ahead, "waves": waves,
                                   "by_cols": hist[0], "by_blocks": hist[1], "by_outside": hist[2], "inside": int(m.group(11)), "outside": int(m.group(12))}
        assert sum(hist[0].values()) == tasks
    return stages


def parse_launches(err):
    """What launch_backward_simt says per launch under SLAMPP_HIP_STAGE_TIMING: [(chunks, width, block size, members, fetch ahead)]."""
    return [(int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)), m.group(5) == "fetch ahead")
            for m in re.finditer(r"stage_timing lane-per-task backward launch: (\d+) chunks, width (\d+), block size (\d+), (\d+) members, "
                                 r"(fetch ahead|fetch by column)", err)]


def analyzed(monkeypatch, capfd, case):
    from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP
    name, options = CASES[case]
    monkeypatch.setenv("SLAMPP_HIP_DEV", "1")
    monkeypatch.setenv("SLAMPP_HIP_PLAN_TIMING", "1")
    monkeypatch.setenv("SLAMPP_HIP_STAGE_TIMING", "1")     # (read at analysis: the launches then say which form they take)
    sysrec = system(name)
    solver = CLinearSolver_HIP(**dict(options, **LANES))
    capfd.readouterr()
    assert solver.SymbolicDecomposition_Blocky(sysrec.lam)
    _reached[case] = parse_report(capfd.readouterr().err)
    monkeypatch.delenv("SLAMPP_HIP_PLAN_TIMING")
    assert 0 in _reached[case], "the leaf stage has no lane-per-task chunks"
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


def check_launches(launches, value, stage, members):
    """Every lane-per-task backward launch took the form the knob asks for: 0 = by column, 1 = ahead, unset = ahead where the
    launch fits one round of the fetch-ahead form (the stage's waves, asked at analysis)."""
    assert launches
    for chunks, width, d, n_members, ahead in launches:
        assert (chunks, width, d, n_members) == (stage["chunks"], stage["width"], 6, members), launches
        want = {0: False, 1: True, None: chunks * members <= stage["waves"]}[value]
        assert ahead == want, (value, launches, stage)


@pytest.mark.parametrize("case", sorted(CASES))
def test_bit_equal_to_the_fetch_by_column(monkeypatch, capfd, case):
    sysrec, solver = analyzed(monkeypatch, capfd, case)
    lam, x_ref, stage = sysrec.lam, sysrec.x_ref, _reached[case][0]
    assert stage["waves"] > 0 and stage["chunks"] * 3 <= stage["waves"]    # (the small launches below are small by the rule)
    # (the first kept-factor solve of a handle takes inv(L_jj) of the leaf columns from invert_diagonals_kernel, every later one
    # from the factor kernel, which stores them from then on -- last bits apart, whatever the knob says: one round before the
    # comparison puts every value of the knob on the same footing)
    eta = lam.rhs.copy()
    assert solver.Solve_PosDef_Blocky(lam, eta) and solver.Solve_Again(eta)
    got = {}
    for value in (0, 1, None):
        if value is None:
            monkeypatch.delenv(KNOB)
        else:
            monkeypatch.setenv(KNOB, str(value))
        capfd.readouterr()
        eta = lam.rhs.copy()
        assert solver.Solve_PosDef_Blocky(lam, eta) and V.rel_inf(eta, x_ref) < V.TOL
        check_launches(parse_launches(capfd.readouterr().err), value, stage, 1)
        again = -2.0 * lam.rhs                              # a second right-hand side on the kept factor
        assert solver.Solve_Again(again) and V.rel_inf(again, -2.0 * x_ref) < V.TOL
        check_launches(parse_launches(capfd.readouterr().err), value, stage, 1)
        x_batch = batch(solver, lam, x_ref, 3)              # the member strides
        check_launches(parse_launches(capfd.readouterr().err), value, stage, 3)
        got[value] = (eta, again, x_batch)
    for value in (1, None):
        for x0, x1 in zip(got[0], got[value]):
            assert np.array_equal(x0, x1)


def test_a_batch_beyond_one_round_keeps_the_fetch_by_column(monkeypatch, capfd):
    """Unset, the knob leaves a launch of more waves than one round of the fetch-ahead form holds to backward_simt_kernel; at 1
    the same batch takes the fetch-ahead form and gives the same bits."""
    sysrec, solver = analyzed(monkeypatch, capfd, "chain_short")
    lam, x_ref, stage = sysrec.lam, sysrec.x_ref, _reached["chain_short"][0]
    K = stage["waves"] // stage["chunks"] + 1
    assert stage["waves"] > 0 and stage["chunks"] * K > stage["waves"] and K <= 256, stage
    got = {}
    for value in (None, 1):
        if value is not None:
            monkeypatch.setenv(KNOB, str(value))
        capfd.readouterr()
        got[value] = batch(solver, lam, x_ref, K)
        check_launches(parse_launches(capfd.readouterr().err), value, stage, K)
    assert np.array_equal(got[None], got[1])


@pytest.mark.parametrize("name", ["chain3", "chain7"])
def test_odd_block_sizes_solve_on_the_kernel_they_take(monkeypatch, name):
    r = V.run_variant(monkeypatch, name, LANES, {"SLAMPP_HIP_DEV": 1, KNOB: 1}, [])
    assert r.simt_stage_count() >= 1 and r.opt("simt_backward", -1) == 1     # (the leaf stage went to the lane-per-task kernels)


def test_the_cases_reach_the_column_loops_edges(monkeypatch, capfd):
    """Over the cases together: tasks of one column (prologue only), of two and of three (both parities of the unrolled loop's
    tail) and of eight; columns with no block below the diagonal (the islands' last columns), with exactly as many as a register
    set holds and with more (the batches inside the column); rows inside the task and outside; chunks with spare lanes -- read
    from the analysis of each case (the ones the equality tests have not run yet are analyzed here)."""
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
    assert any(n > 0 for s in stages for b, n in s["by_blocks"].items() if b > ahead), stages
    assert any(n > 0 for s in stages for b, n in s["by_blocks"].items() if b > 2 * ahead), stages   # more than one batch inside the column
    assert any(s["inside"] > 0 for s in stages) and any(s["outside"] > 0 for s in stages)
    # a register set holds x of one row outside the task: columns with none among the set's blocks (the load is a stand-in), with
    # one, and with more (the others are fetched inside the column)
    for n_outside in (0, 1, 2):
        assert any(s["by_outside"].get(n_outside, 0) > 0 for s in stages), (n_outside, stages)
    assert any(s["spare"] > 0 for s in stages)
