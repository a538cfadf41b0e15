"""The packed operand fetch of the panel tasks (csrc/panel_kernel.hip: panel_fetch_packed; knob SLAMPP_HIP_DEV_PANEL_FETCH):
the operand blocks of the products a task brings in itself travel as 16-byte loads, three 6 x 6 blocks per instruction, a
group of products in flight per wave, and go through the same staging area in passes of three products.  The products and
sums are the ones the block-per-instruction fetch performs, in the same order, so the results are required to be
bit-identical (np.array_equal, no tolerance): the factor and the solutions of one handle with the knob at 0 and at 1, and
the members of a batch.  Every case also goes through the full list of variant checks (tests/variant_util.py: run_variant)
with the knob at 1, the stage lines of SLAMPP_HIP_PLAN_TIMING say what the cases reach, and the launch lines of
SLAMPP_HIP_STAGE_TIMING which fetch every panel launch took (unset, the knob leaves the packed fetch to two waves a task)."""
import re

import numpy as np
import pytest

import variant_util as V

pytestmark = pytest.mark.gpu

KNOB = "SLAMPP_HIP_DEV_PANEL_FETCH"
W4, W2 = "SLAMPP_HIP_DEV_PANEL_W4_MIN", "SLAMPP_HIP_DEV_PANEL_W2_MIN"
PASS = {2: 3, 4: 6, 8: 3}                 # products per pass by waves a task (sparse_kernels.h: panel_fetch_pass)
GROUP = {2: 9, 4: 12, 8: 6}               # products in flight per wave (sparse_kernels.h: panel_fetch_group)

# name -> (system, options on top of PLAN_OPTIONS, knobs)
CASES = {
    "a_simt": ("chain6", {"simt": 1}, {}),                              # a b_from_lambda stage right above lane-per-task leaves
    "b_simt_w2": ("chain6", {"simt": 1}, {W2: 0}),
    "b_simt_w4": ("chain6", {"simt": 1}, {W4: 0}),
    "c_defaults": ("chain6", {}, {}),                                   # riders in the launch below
    "d_no_riders": ("chain6", {}, {"SLAMPP_HIP_DEV_PANEL_RIDE_FRESH": 0}),   # panel_update_kernel on its own
    "e_no_handup": ("chain6", {"panel_handup": 0}, {}),                 # the upper stages fetch their products themselves
    "f_hub": ("hub", {}, {}),
    "f_sphere": ("sphere", {}, {}),
    "g_hub_w4": ("hub", {"simt": 1}, {W4: 0}),                          # four waves a task with more than one group per wave
}

_reached = {}                             # case -> what its analysis reported (parse_setup)


def parse_setup(err):
    """The lines CPanelPass (sparse_records.cpp) prints per stage under SLAMPP_HIP_PLAN_TIMING: {stage: {"waves", "pass", "min", "max",
    "mod": waves by count modulo the stage's pass size, "few": waves with fewer entries than a pass, by count}} and the stages
    whose tasks bring in all their updates themselves."""
    fetch, self_fetched = {}, set()
    for m in re.finditer(r"\[setup\] stage (\d+) fresh fetch: (\d+) waves a task, pass of (\d+), (\d+) to (\d+) self-fetched entries per wave; "
                         r"waves by entries modulo the pass:((?: \d+)+); waves with fewer than a pass, by entries:((?: \d+)+)", err):
        stage, waves, n_pass, lo, hi = map(int, m.groups()[:5])
        mod, few = ([int(v) for v in g.split()] for g in m.groups()[5:])
        assert n_pass == PASS[waves] and len(mod) == n_pass and len(few) == n_pass
        fetch[stage] = {"waves": waves, "pass": n_pass, "min": lo, "max": hi, "mod": mod, "few": few}
    for m in re.finditer(r"\[setup\] stage (\d+): \d+ tasks, .*: the tasks bring them in", err):
        self_fetched.add(int(m.group(1)))
    return fetch, self_fetched


def parse_launches(err):
    """What launch_factor_panel (panel_kernel.hip) says per launch under SLAMPP_HIP_STAGE_TIMING: [(waves a task, fused, packed)]
    of the launches with the fixed block size 6."""
    return [(int(m.group(1)), int(m.group(3)) != 0, m.group(4) == "packed")
            for m in re.finditer(r"stage_timing panel launch: \d+ tasks, (\d+) waves a task, block size (\d+), fused (\d+), fetch (packed|block per load)", err)
            if int(m.group(2)) == 6]


def analyzed(monkeypatch, capfd, case):
    """A handle of the case, analyzed with SLAMPP_HIP_PLAN_TIMING set; what the record builders said is kept for the reach test."""
    from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP
    name, options, knobs = CASES[case]
    for k, v in knobs.items():
        monkeypatch.setenv(k, str(v))
    monkeypatch.setenv("SLAMPP_HIP_PLAN_TIMING", "1")
    monkeypatch.setenv("SLAMPP_HIP_STAGE_TIMING", "1")     # (read at analysis: the launches then say which fetch they take)
    sysrec = V.system(name)
    solver = CLinearSolver_HIP(**dict(V.PLAN_OPTIONS, **options))
    capfd.readouterr()
    assert solver.SymbolicDecomposition_Blocky(sysrec.lam)
    _reached[case] = parse_setup(capfd.readouterr().err)
    monkeypatch.delenv("SLAMPP_HIP_PLAN_TIMING")
    fetch, self_fetched = _reached[case]
    assert fetch, "no panel stage"
    assert sysrec.d == 6
    if case.startswith(("a_", "b_", "e_")):                # (with hand-ups a chain's upper stages may fetch nothing themselves)
        assert any(f["max"] > 0 for f in fetch.values()), "no panel stage fetches a product itself"
    if case.startswith(("a_", "b_")):
        assert self_fetched, "no stage whose tasks bring in all their updates (b_from_lambda)"
    want = {"b_simt_w2": 2, "b_simt_w4": 4, "g_hub_w4": 4}.get(case)
    if want:
        assert any(f["waves"] == want and f["max"] > 0 for f in fetch.values()), fetch
    return sysrec, solver


def batch(solver, sysrec):
    import torch
    lam = sysrec.lam
    K = len(V.ALPHAS)
    sv, sr = lam.values.shape[0] + 6, lam.n_scalars + 6
    sv, sr = sv + sv % 2, sr + sr % 2                       # even strides: one pass of launches, the member from blockIdx.y
    vals = torch.zeros(K * sv, dtype=torch.float64, device="cuda")
    rhs = torch.zeros(K * sr, dtype=torch.float64, device="cuda")
    for k, a in enumerate(V.ALPHAS):
        vals[k * sv:k * sv + lam.values.shape[0]] = torch.from_numpy(sysrec.member(a)[0].values).cuda()
        rhs[k * sr:k * sr + lam.n_scalars] = torch.from_numpy((k + 1.0) * lam.rhs).cuda()
    torch.cuda.synchronize()
    solver.factor_solve_batch_device_async(K, vals.data_ptr(), sv, rhs.data_ptr(), sr)
    assert solver.sync_batch(K) == [True] * K
    x = rhs.cpu().numpy()
    for k, a in enumerate(V.ALPHAS):
        assert V.rel_inf(x[k * sr:k * sr + lam.n_scalars], (k + 1.0) * sysrec.member(a)[1]) < V.TOL, (k, a)
    return x


def check_launches(launches, value, fetches):
    """The fused launches took the fetch the knob asks for: 0 = none packed, 1 = all, unset = those of two waves a task."""
    fused = [(w, packed) for w, b_fused, packed in launches if b_fused]
    assert all(not packed for w, b_fused, packed in launches if not b_fused)
    if fetches:
        assert fused, launches
    for w, packed in fused:
        assert packed == {0: False, 1: True, None: w == 2}[value], (value, launches)


@pytest.mark.parametrize("case", sorted(CASES))
def test_bit_equal_to_the_block_per_load_fetch(monkeypatch, capfd, case):
    sysrec, solver = analyzed(monkeypatch, capfd, case)
    fetches = any(f["max"] > 0 for f in _reached[case][0].values())
    lam = sysrec.lam
    got = {}
    for value in (0, 1, None):
        if value is None:
            monkeypatch.delenv(KNOB)
        else:
            monkeypatch.setenv(KNOB, str(value))
        capfd.readouterr()
        ok, st, l_values = solver.factorize(lam)
        assert ok
        check_launches(parse_launches(capfd.readouterr().err), value, fetches)
        V.check_factor(sysrec, st, l_values)
        eta = lam.rhs.copy()
        assert solver.Solve_PosDef_Blocky(lam, eta) and V.rel_inf(eta, sysrec.x_ref) < V.TOL
        x_batch = batch(solver, sysrec)
        check_launches(parse_launches(capfd.readouterr().err), value, fetches)
        got[value] = (np.array(l_values), eta, x_batch)
    for value in (1, None):
        for x0, x1 in zip(got[0], got[value]):
            assert np.array_equal(x0, x1)


@pytest.mark.parametrize("case", sorted(CASES))
def test_variant_checks_with_the_packed_fetch(monkeypatch, case):
    name, options, knobs = CASES[case]
    V.run_variant(monkeypatch, name, options, dict(knobs, **{KNOB: 1}), [])


@pytest.mark.parametrize("name", ["chain3", "chain7"])
def test_odd_block_sizes_keep_their_path(monkeypatch, name):
    V.run_variant(monkeypatch, name, {"simt": 1}, {KNOB: 1}, [])


def test_the_cases_reach_the_fetch_loops_edges(monkeypatch, capfd):
    """Over the cases together some wave fetches no product itself, one, fewer than a pass, more than two groups, and every
    count modulo the pass size of three (two and eight waves a task; at four the pass is six: its edges below) -- read from the analysis of each case (the ones the equality tests have not run yet are
    analyzed here)."""
    for case in sorted(CASES):
        if case not in _reached:
            analyzed(monkeypatch, capfd, case)
    stages = [f for case in sorted(CASES) for f in _reached[case][0].values()]
    assert any(f["few"][0] > 0 for f in stages)                                  # none
    assert any(f["few"][1] > 0 for f in stages)                                  # one
    assert any(sum(f["few"][1:]) > 0 for f in stages)                            # fewer than one pass
    assert any(f["max"] > 2 * GROUP[f["waves"]] for f in stages), stages         # more than two groups
    for waves in (2, 8):                                                         # pass of three: every residue, beyond the first pass too
        mine = [f for f in stages if f["waves"] == waves]
        for residue in range(PASS[waves]):
            assert any(f["mod"][residue] > f["few"][residue] for f in mine), (waves, residue, mine)
    mine = [f for f in stages if f["waves"] == 4]                                # pass of six (two load pairs of three products):
    assert any(f["max"] > GROUP[4] for f in mine), mine                          # more than one group,
    assert any(sum(f["mod"][1:3]) + sum(f["mod"][4:6]) > 0 for f in mine), mine  # a last load pair that is not full
    assert any(sum(f["mod"][1:]) > 0 for f in mine), mine                        # and a last pass that is not full
    assert _reached["a_simt"][1], "case (a): no stage whose tasks bring in all their updates"
