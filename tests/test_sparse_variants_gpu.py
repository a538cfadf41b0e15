"""Every size-gated branch of the sparse block Cholesky (csrc/sparse_enqueue.hip runs a schedule, not a kernel) at a few hundred
poses: the options and development knobs that pick a kernel instantiation are set explicitly, the test proves from plan(),
stats() and profile() that the instantiation ran (a case whose reach predicate is false fails), and checks the factor block by
block against numpy's dense Cholesky, the solves against a refined fp64 solution, batches member by member and that a
failure planted in the variant's own stage surfaces.  variant_util.py holds the systems, references, gates and checks;
DESIGN.md ("Which test guards which branch") maps branch -> gate -> test id."""
import pytest

import variant_util as V

pytestmark = pytest.mark.gpu

CHAINS = ["chain3", "chain6", "chain7"]
W4, W2 = "SLAMPP_HIP_DEV_PANEL_W4_MIN", "SLAMPP_HIP_DEV_PANEL_W2_MIN"
PAIRS = "SLAMPP_HIP_DEV_SIMT_PAIRS"


def first_wide_stage(r):
    return max(r.simt_stage_count(), 1)


def first_separator_stage(r):
    return min(r.n_bottom, r.n_stages - 1)


# ---- gates 1 and 2: the wide stages (one wave per column, factor_stage_kernel<D, 1, WIDE_CHUNK, WIDE_NR, WIDE_NP>) -----------

@pytest.mark.parametrize("wide_min", [1, 8])
@pytest.mark.parametrize("name", CHAINS + ["sphere"])
def test_wide_stages(monkeypatch, name, wide_min):
    V.run_variant(monkeypatch, name, {"wide_min_tasks": wide_min}, {}, [V.reach_wide], stage_of=first_wide_stage, natural=True,
                  profile_phase="factor_wide")


@pytest.mark.parametrize("wide_min", [1, 8])
def test_wide_stages_with_columns_over_the_package_limits(monkeypatch, wide_min):
    V.run_variant(monkeypatch, "hub", {"wide_min_tasks": wide_min}, {}, [V.reach_wide_packages], stage_of=first_wide_stage,
                  natural=True, profile_phase="factor_wide")


@pytest.mark.parametrize("wide_min", [1, 8])
def test_wide_stages_of_mixed_block_sizes(monkeypatch, wide_min):
    V.run_variant(monkeypatch, "mixed", {"wide_min_tasks": wide_min}, {}, [V.reach_wide_mixed], stage_of=lambda r: 1, natural=True,
                  profile_phase="factor_wide")


@pytest.mark.parametrize("panel", [1, 0])
@pytest.mark.parametrize("simt", [0, 1])
@pytest.mark.parametrize("wide_min", [1, 8])
def test_wide_stages_beside_the_other_leaf_and_separator_kernels(monkeypatch, wide_min, simt, panel):
    V.run_variant(monkeypatch, "chain6", {"wide_min_tasks": wide_min, "simt": simt, "panel": panel}, {PAIRS: 1},
                  [V.reach_wide] + ([V.reach_simt] if simt else []), stage_of=first_wide_stage, natural=True, profile_phase="factor_wide")


# ---- gates 3 and 4: the lane-per-task kernels (factor_simt_kernel<D, W, LPT, StoreLinv>, backward_simt_kernel<D, W>) ---------

@pytest.mark.parametrize("backward", [0, 1])
@pytest.mark.parametrize("pairs", [0, 1])
@pytest.mark.parametrize("width", [16, 32, 64])
@pytest.mark.parametrize("name", CHAINS)
def test_lane_per_task_leaves(monkeypatch, name, width, pairs, backward):
    r = V.run_variant(monkeypatch, name, {"simt": 1, "simt_width": width, "simt_backward": backward}, {PAIRS: pairs},
                      [V.reach_simt_backward if backward else V.reach_simt])
    assert r.lanes_per_task == (2 if pairs and name == "chain6" and width <= 32 else 1)


@pytest.mark.parametrize("pairs", [0, 1])
@pytest.mark.parametrize("stages", [2, 3])
@pytest.mark.parametrize("name", CHAINS)
def test_lane_per_task_stages_above_the_leaves(monkeypatch, name, stages, pairs):
    V.run_variant(monkeypatch, name, {"simt": 1, "simt_width": 32, "simt_stages": stages, "wide_min_tasks": 8}, {PAIRS: pairs},
                  [V.reach_simt, V.reach_simt_stages, V.reach_wide], stage_of=lambda r: 1, profile_phase="factor_wide")


# ---- gate 7: the panel launch shapes ---------------------------------------------------------------------------------------------

PANEL_CASES = {
    "w4": ({}, {W4: 0}, [V.reach_panel_waves(4)]),
    "w2": ({}, {W2: 0}, [V.reach_panel_waves(2)]),
    "w4_rows0": ({"panel_rows": 0}, {W4: 0}, [V.reach_panel_waves(4)]),
    "w4_rows1": ({"panel_rows": 1}, {W4: 0}, [V.reach_panel_waves(4)]),
    "w2_rows0": ({"panel_rows": 0}, {W2: 0}, [V.reach_panel_waves(2)]),
    "w2_rows1": ({"panel_rows": 1}, {W2: 0}, [V.reach_panel_waves(2)]),
    "no_riders": ({}, {"SLAMPP_HIP_DEV_PANEL_RIDE_FRESH": 0}, [V.reach_panel_no_riders]),
    "handup_narrow": ({}, {"SLAMPP_HIP_DEV_HANDUP_MAX_TASKS": 4}, [V.reach_handup_narrow]),
    # (the crowded branch itself, b_below_crowded in CPanelPass::Decide_Stage() of sparse_records.cpp, wants more than 1 024 panel tasks in the stage below: the knob is set and
    # the two-wave launch it is listed with is what is reached at this size)
    "self_above_crowded_w2": ({}, {"SLAMPP_HIP_DEV_PANEL_SELF_ABOVE_CROWDED": 1, W2: 0}, [V.reach_panel_waves(2)]),
    "max_cols_2": ({}, {"SLAMPP_HIP_DEV_TASK_MAX_COLS": 2}, [V.reach_task_caps]),
    "max_blocks_1": ({}, {"SLAMPP_HIP_DEV_TASK_MAX_BLOCKS": 1}, [V.reach_task_caps]),   # (1: the knob's floor, plan.cpp:1347)
    # (simt = 0 alone leaves few leaf tasks to the panel kernel, b_leaf_panels in CPanelPass::Run() of sparse_records.cpp: panel = 0 takes them to launch_factor_stage)
    "subtree_v1": ({"simt": 0, "panel": 0}, {"SLAMPP_HIP_DEV_SUBTREE_V1": 1}, [V.reach_subtree_v1]),
}


@pytest.mark.parametrize("case", sorted(PANEL_CASES))
@pytest.mark.parametrize("name", ["chain6", "sphere"])
def test_panel_launch_shapes(monkeypatch, name, case):
    options, knobs, reaches = PANEL_CASES[case]
    V.run_variant(monkeypatch, name, options, knobs, reaches, stage_of=(lambda r: 0) if case == "subtree_v1" else first_separator_stage)


# ---- gate 5 and the schedule a million-pose graph gets, at 600 poses ----------------------------------------------------------

@pytest.mark.parametrize("name", CHAINS)
def test_the_schedule_of_a_large_graph_at_small_size(monkeypatch, name):
    V.run_variant(monkeypatch, name, {"simt": 1, "simt_backward": 1, "wide_min_tasks": 8}, {PAIRS: 0, W4: 0, W2: 0},
                  [V.reach_simt_backward, V.reach_wide, V.reach_panel_waves(2)], stage_of=first_wide_stage, alphas=V.ALPHAS_8,
                  profile_phase="factor_wide")


# ---- gate 6: pointers that are 8-byte aligned only ----------------------------------------------------------------------------------

@pytest.mark.parametrize("backward", [0, 1])
@pytest.mark.parametrize("name", ["chain6", "chain3"])
def test_misaligned_device_pointers(monkeypatch, name, backward):
    V.run_misaligned(monkeypatch, name, {"simt": 1, "simt_backward": backward})
