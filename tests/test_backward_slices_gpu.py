"""backward_slice_kernel (csrc/sparse_kernels.hip; option panel_backward): the backward substitution of the tasks the panel
kernel factored, one trip to memory per task.  Per column it performs backward_stage_kernel's operations in the same
order, so its results are required to be bit-identical to that kernel's (np.array_equal, no tolerance): on one handle and
one kept factor, the same right-hand side solved with panel_backward = 0 and = 1, and whole factor-and-solve calls either
way.  The full list of variant checks (tests/variant_util.py: run_variant) runs with the option forced on."""
import re

import numpy as np
import pytest

import variant_util as V

pytestmark = pytest.mark.gpu

CHAINS = ["chain3", "chain6", "chain7"]
W4 = "SLAMPP_HIP_DEV_PANEL_W4_MIN"      # (as tests/test_sparse_variants_gpu.py sets it: 0 = every panel stage a crowded one)


def hub_clique(d):
    """The chain, hub and banded stretch of variant_util's hub_chain with a clique of 110 vertices hanging off pose 150 (as in tests/backward_records_driver.cpp):
    the clique's first columns have more blocks than a panel image has slots, so a panel stage holds tasks left to the
    column kernel beside packaged ones, and the hub's neighbours are packaged columns with more than nine blocks."""
    from slam_plus_plus_amd import synth
    n, n_clique = 300, 110
    rng = np.random.default_rng(71)
    ci = np.arange(n - 1)
    ends = np.arange(50, n, 50)
    li = ends - rng.integers(26, 51, size=len(ends))
    band = np.arange(180, 260)
    iu, ju = np.triu_indices(n_clique, 1)
    ei = [ci, li, np.arange(10, 70), band, band, np.full(n_clique, 150), n + 1 + iu]
    ej = [ci + 1, ends, np.full(60, n), band + 2, band + 3, n + 1 + np.arange(n_clique), n + 1 + ju]
    return synth._assemble_pose_graph(n + 1 + n_clique, d, np.concatenate(ei), np.concatenate(ej), rng, 0.02, 100.0, f"hub_clique{d}")


V.SYSTEMS.setdefault("hub_clique6", lambda: hub_clique(6))      # (variant_util.system() builds and keeps them with their references)
V.SYSTEMS.setdefault("hub_clique3", lambda: hub_clique(3))


def analyzed(monkeypatch, capfd, solver, lam):
    """Analyzes with SLAMPP_HIP_PLAN_TIMING set and returns what the record builders said they made (CPanelPass::Run() in
    sparse_records.cpp prints it): {stage: {"tasks", "units", "blocks", "levels", "cols_per_wave"}} of the backward records
    and {stage: tasks left to the column kernel}."""
    monkeypatch.setenv("SLAMPP_HIP_PLAN_TIMING", "1")
    capfd.readouterr()
    assert solver.SymbolicDecomposition_Blocky(lam)
    return parse_setup(capfd.readouterr().err)


def parse_setup(err):
    records, rest = {}, {}
    for m in re.finditer(r"\[setup\] stage (\d+) backward records: (\d+) tasks, at most (\d+) units, (\d+) blocks below a diagonal and (\d+) levels per task; (\d+) columns per wave", err):
        records[int(m.group(1))] = dict(zip(("tasks", "units", "blocks", "levels", "cols_per_wave"), map(int, m.groups()[1:])))
    for m in re.finditer(r"\[setup\] stage (\d+) panels: .* (\d+) tasks left to the column kernel", err):
        rest[int(m.group(1))] = int(m.group(2))
    return records, rest


def task_levels(plan, t):
    """Levels of task t: 1 + the longest chain of its columns in which each has a block in the row of the next."""
    cols = plan["task_cols"][plan["task_ptr"][t]:plan["task_ptr"][t + 1]].tolist()
    inside = set(cols)
    depth = {}
    for j in reversed(cols):                          # (rows of a column come later in the task's order)
        rows = [int(i) for i in plan["lrow"][plan["lptr"][j] + 1:plan["lptr"][j + 1]] if int(i) in inside]
        depth[j] = 1 + max((depth[i] for i in rows), default=0)
    return max(depth.values())


def reach_slices(r):
    """sparse_enqueue.hip, the backward loop: a stage takes backward_slice_kernel if it was factored as panels
    (lists.panel_ptr[s + 1] > lists.panel_ptr[s]), the block size is 3, 6 or 7 and panel_backward != 0.  At least two such
    stages, and a task of two or more levels (a barrier between levels, x handed on through LDS)."""
    assert r.opt("panel_backward", -1) != 0 and r.fixed_dim
    ps = r.panel_stages()
    assert len(ps) >= 2, ps
    assert any(task_levels(r.plan, t) >= 2 for s in ps for t in range(r.plan["stage_ptr"][s], r.plan["stage_ptr"][s + 1]))


def last_panel_stage(r):
    return r.panel_stages()[-1]


# ---- 1. every check of a variant with the new kernel forced on ----------------------------------------------------------------

@pytest.mark.parametrize("name", CHAINS)
def test_variant_checks_with_backward_slices(monkeypatch, name):
    V.run_variant(monkeypatch, name, {"panel_backward": 1}, {}, [reach_slices], stage_of=last_panel_stage, profile_phase="backward")


# ---- 2 - 4. bit equality with backward_stage_kernel -----------------------------------------------------------------------------

def both_ways(solver, lam, x_ref):
    """One kept factor, the same right-hand side with panel_backward 0 and 1; then whole solves either way."""
    out = {}
    solver.set_option("panel_backward", 0)
    eta = lam.rhs.copy()
    assert solver.Solve_PosDef_Blocky(lam, eta) and V.rel_inf(eta, x_ref) < V.TOL
    out["full0"] = eta
    for value in (0, 1, 0):
        solver.set_option("panel_backward", value)
        eta = 3.0 * lam.rhs
        assert solver.Solve_Again(eta) and V.rel_inf(eta, 3.0 * x_ref) < V.TOL
        out.setdefault(f"again{value}", eta)
        assert np.array_equal(eta, out[f"again{value}"])          # (the same kernel twice: the same bits)
    solver.set_option("panel_backward", 1)
    eta = lam.rhs.copy()
    assert solver.Solve_PosDef_Blocky(lam, eta) and V.rel_inf(eta, x_ref) < V.TOL
    out["full1"] = eta
    assert np.array_equal(out["again0"], out["again1"])
    assert np.array_equal(out["full0"], out["full1"])


# name -> (system, options, knobs, what the analysis must report: "nine" = a packaged column with more than nine blocks (the
# kernel's loop over the blocks beyond the lane groups' first), "rest" = a stage with packaged tasks and tasks left to the
# column kernel (the second launch through task_map), 1 / 2 / 4 = columns per wave of some stage)
EQUALITY_CASES = {
    "chain3": ("chain3", V.PLAN_OPTIONS, {}, [1]),
    "chain6": ("chain6", V.PLAN_OPTIONS, {}, [1]),
    "chain7": ("chain7", V.PLAN_OPTIONS, {}, [1]),
    "hub": ("hub", V.PLAN_OPTIONS, {}, ["nine"]),
    "hub_clique6": ("hub_clique6", V.PLAN_OPTIONS, {}, ["nine", "rest"]),
    "hub_clique3": ("hub_clique3", V.PLAN_OPTIONS, {}, ["nine", "rest"]),
    "sphere": ("sphere", V.PLAN_OPTIONS, {}, [1]),
    "sphere_default": ("sphere", {}, {}, [1]),
    "chain6_w4": ("chain6", V.PLAN_OPTIONS, {W4: 0}, [2]),       # 3. two columns per wave
    "chain7_w2": ("chain7", V.PLAN_OPTIONS, {W4: 0, "SLAMPP_HIP_DEV_PANEL_W2_MIN": 0}, [4]),
}


def check_reach(records, rest, wanted):
    assert records, "no stage has backward records: the slice kernel has nothing to take"
    for want in wanted:
        if want == "nine":
            assert any(r["blocks"] > 8 for r in records.values()), records          # (blocks below the diagonal: nb - 1)
        elif want == "rest":
            assert any(rest.get(s, 0) > 0 for s in records), (records, rest)
        else:
            assert any(r["cols_per_wave"] == want for r in records.values()), records
    assert any(r["levels"] >= 2 for r in records.values()), records


@pytest.mark.parametrize("case", sorted(EQUALITY_CASES))
def test_bit_equal_to_the_column_kernel(monkeypatch, capfd, case):
    from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP
    name, options, knobs, wanted = EQUALITY_CASES[case]
    for k, v in knobs.items():
        monkeypatch.setenv(k, str(v))
    sysrec = V.system(name)
    solver = CLinearSolver_HIP(**options)
    records, rest = analyzed(monkeypatch, capfd, solver, sysrec.lam)
    r = V.Reach(sysrec, dict(options), dict(knobs), solver.plan(), solver.stats())
    assert set(records) <= set(r.panel_stages())
    check_reach(records, rest, wanted)
    both_ways(solver, sysrec.lam, sysrec.x_ref)


def test_default_rule_by_stage_size(monkeypatch):
    """panel_backward = -1 (the default) takes the new kernel in stages of at most SLAMPP_HIP_DEV_BWD_SLICE_MAX_TASKS tasks
    (1 024; sparse_enqueue.hip) and the column kernel in the others.  With the line at 8 the plan has panel stages on either
    side of it; the result is the column kernel's, bit for bit."""
    from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP
    monkeypatch.setenv("SLAMPP_HIP_DEV_BWD_SLICE_MAX_TASKS", "8")
    sysrec = V.system("chain6")
    lam = sysrec.lam
    solver = CLinearSolver_HIP(**V.PLAN_OPTIONS)
    assert solver.SymbolicDecomposition_Blocky(lam)
    r = V.Reach(sysrec, dict(V.PLAN_OPTIONS), {}, solver.plan(), solver.stats())
    sizes = [V.stage_tasks(r.plan, s) for s in r.panel_stages()]
    assert any(n <= 8 for n in sizes) and any(n > 8 for n in sizes), sizes
    got = {}
    for value in (0, -1):
        solver.set_option("panel_backward", value)
        eta = lam.rhs.copy()
        assert solver.Solve_PosDef_Blocky(lam, eta) and V.rel_inf(eta, sysrec.x_ref) < V.TOL
        got[value] = eta
    assert np.array_equal(got[0], got[-1])


def test_bit_equal_below_a_dense_top(monkeypatch, capfd):
    """Default options on a sphere large enough for a dense top: the block stages below it read x of the dense top's rows
    from the workspace."""
    from slam_plus_plus_amd import synth
    from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP
    lam = synth.sphere(24, 24, seed=45)
    solver = CLinearSolver_HIP()
    records, rest = analyzed(monkeypatch, capfd, solver, lam)
    assert solver.plan()["dense_dim"] > 0 and solver.stats()["n_stages"] >= 2
    check_reach(records, rest, [])                          # block stages with backward records below the dense top
    both_ways(solver, lam, V.refined_solution(lam))


def test_mixed_block_sizes_step_aside():
    """No fixed block size: no panel packages, no backward records (b_Package_Dim() in sparse_records.cpp), so the option
    changes nothing -- asserted through the plan -- and the results are equal trivially."""
    from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP
    sysrec = V.system("mixed")
    solver = CLinearSolver_HIP(**V.PLAN_OPTIONS)
    assert solver.SymbolicDecomposition_Blocky(sysrec.lam)
    r = V.Reach(sysrec, dict(V.PLAN_OPTIONS), {}, solver.plan(), solver.stats())
    assert not r.fixed_dim and r.panel_stages() == []
    both_ways(solver, sysrec.lam, sysrec.x_ref)


@pytest.mark.parametrize("name", ["chain6", "chain3", "chain7", "hub", "hub_clique6", "sphere"])
def test_batch_members_bit_equal(monkeypatch, capfd, name):
    import torch
    from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP
    sysrec = V.system(name)
    lam = sysrec.lam
    solver = CLinearSolver_HIP(**V.PLAN_OPTIONS)
    records, rest = analyzed(monkeypatch, capfd, solver, lam)
    check_reach(records, rest, {"hub": ["nine"], "hub_clique6": ["nine", "rest"]}.get(name, []))
    V.reach_batch(V.Reach(sysrec, dict(V.PLAN_OPTIONS), {}, solver.plan(), solver.stats()))
    K = len(V.ALPHAS)
    sv, sr = lam.values.shape[0] + 6, lam.n_scalars + 6
    sv, sr = sv + sv % 2, sr + sr % 2                       # even strides: one pass of launches, the member from blockIdx.y
    vals = torch.zeros(K * sv, dtype=torch.float64, device="cuda")
    for k, a in enumerate(V.ALPHAS):
        vals[k * sv:k * sv + lam.values.shape[0]] = torch.from_numpy(sysrec.member(a)[0].values).cuda()
    got = {}
    for value in (0, 1):
        solver.set_option("panel_backward", value)
        rhs = torch.zeros(K * sr, dtype=torch.float64, device="cuda")
        for k in range(K):
            rhs[k * sr:k * sr + lam.n_scalars] = torch.from_numpy((k + 1.0) * lam.rhs).cuda()
        torch.cuda.synchronize()
        solver.factor_solve_batch_device_async(K, vals.data_ptr(), sv, rhs.data_ptr(), sr)
        assert solver.sync_batch(K) == [True] * K
        got[value] = rhs.cpu().numpy()
    for k, a in enumerate(V.ALPHAS):
        x0, x1 = (got[v][k * sr:k * sr + lam.n_scalars] for v in (0, 1))
        assert V.rel_inf(x1, (k + 1.0) * sysrec.member(a)[1]) < V.TOL, (k, a)
        assert np.array_equal(x0, x1), (k, a)


# ---- 5. vectors that are 8-byte aligned only ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["chain6", "chain3"])
def test_misaligned_vectors_with_backward_slices(monkeypatch, name):
    V.run_misaligned(monkeypatch, name, {"simt": 1, "panel_backward": 1})


# ---- 6. Schur mode: the reduced camera system through the sparse block path -----------------------------------------------------

def test_schur_reduced_system_bit_equal(monkeypatch, capfd):
    from slam_plus_plus_amd import synth
    from slam_plus_plus_amd.hip_solver import CLinearSolver_Schur_HIP
    from oracle import oracle_lib as O
    lam = synth.ba(60, 3000, k=4, mode="band", seed=777)
    ok, x_ref, _, _ = O.solve_schur(lam)
    assert ok
    got = {}
    monkeypatch.setenv("SLAMPP_HIP_PLAN_TIMING", "1")       # (the inner solver's record builders report too)
    for value in (0, 1):
        solver = CLinearSolver_Schur_HIP(schur_sparse=1, dense_top_nb=0, panel_backward=value, profile=1)
        eta = lam.rhs.copy()
        capfd.readouterr()
        assert solver.Solve_PosDef(lam, eta)
        check_reach(*parse_setup(capfd.readouterr().err), [])    # the reduced camera system has stages with backward records
        assert solver.profile().get("reduced_sparse", (0, 0.0))[0] > 0, solver.profile()
        assert solver.reduced_stats()["n_stages"] >= 2
        assert V.rel_inf(eta, x_ref) < V.TOL
        got[value] = eta
    assert np.array_equal(got[0], got[1])
