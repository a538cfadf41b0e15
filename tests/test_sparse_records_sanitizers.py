"""The host record builders of the sparse block path under sanitizers (CPU only).  csrc/sparse_records.cpp depends on
plan.h, sparse_kernels.h and host_pool.h alone and makes no device calls, so it is compiled here with
g++ -fsanitize=address,undefined together with csrc/plan.cpp, csrc/host_pool.cpp and a stand-alone driver
(tests/sparse_records_driver.cpp) that runs the builders in the analysis' order on graphs of a few hundred block columns
and decodes everything they laid out again: every offset inside the array it indexes, every task of a panel stage in
exactly one package or in the rest list, every package as large as its layout, the launches inside the LDS budget, every
update of every packaged factor block delivered exactly once (internal entry, fresh entry, operand pair behind a handed-up
block, or entry of the update lists -- the multiset of operands against the plan's), and every lane of the lane-per-task
tables pointing at the blocks of its own task.  The driver names the branches each case reached; a case that does not
reach the branches listed for it here fails.

The first case is the schedule of a large graph at 600 poses (wide_min_tasks = 8, both wave thresholds at 0).  There the
slice stages begin above wide stages, so none of them is the first stage above the leaves: the stage whose tasks read
Lambda themselves (b_from_lambda) is reached on the same chain with the lane-per-task leaves and the default
wide_min_tasks (chain6-lanes32 / -lanes64).  A task over the package units is reached by a star graph, tasks over the image
by a clique on the hub graph."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam_plus_plus_amd", "csrc")

REACHED = {
    "chain6": {"tall_tasks", "hand_ups", "riders", "launch_order_sorted", "two_waves", "update_launch"},
    "chain6-no-riders": {"tall_tasks", "hand_ups", "update_launch"},
    "chain6-no-hand-ups": {"tall_tasks", "riders", "launch_order_sorted"},
    "chain6-four-waves": {"four_waves", "hand_ups"},
    "chain6-lanes16": {"lane_per_task", "hand_ups"},
    "chain6-lanes32": {"lane_per_task", "b_from_lambda_stage", "hand_ups", "riders", "launch_order_sorted"},
    "chain6-lanes64": {"lane_per_task", "b_from_lambda_stage"},
    "chain6-leaf-panels": {"leaf_panels", "hand_ups", "riders"},
    "chain3": {"leaf_panels", "tall_tasks", "hand_ups"},
    "chain7": {"leaf_panels", "tall_tasks", "hand_ups"},
    "mixed": {"no_column_packages", "no_panel_packages"},
    "chain6-3000": {"upper_first", "hand_ups", "riders"},
    "hub": {"task_over_image", "wide_column_over_limits"},
    "hub-wide8": {"task_over_image", "wide_column_over_limits", "hand_ups"},
    "hub7-leaf-panels": {"task_over_image", "leaf_panels"},
    "star": {"task_over_package_units", "upper_column_over_limits"},
    "grid+dense_top": {"dense_top"},
    "two-chains+dense_top": {"dense_top", "dense_gaps"},
}
NOT_REACHED = {"chain6-no-hand-ups": {"hand_ups"}, "mixed": {"lane_per_task"}}


def test_record_builders_are_right_and_clean_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if not os.path.isfile(os.path.join(rocm, "include", "hip", "hip_runtime.h")):
        pytest.skip("no HIP headers")             # (sparse_kernels.h names longlong2 and hipStream_t)
    exe = tmp_path / "sparse_records_driver"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + CSRC,
           os.path.join(ROOT, "tests", "sparse_records_driver.cpp"), os.path.join(CSRC, "plan.cpp"),
           os.path.join(CSRC, "host_pool.cpp"), os.path.join(CSRC, "sparse_records.cpp"), "-o", str(exe), "-lpthread"]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if build.returncode != 0 and "sanitizer" in (build.stderr or "").lower() and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
    lines = run.stdout.splitlines()
    assert all(l.endswith(" ok") for l in lines), run.stdout
    reached = {l.split(":")[0]: set(l.split(" reached", 1)[1].split()[:-1]) for l in lines}
    assert set(reached) == set(REACHED), run.stdout
    for name, want in REACHED.items():
        assert want <= reached[name], (name, sorted(want - reached[name]))
        assert not (NOT_REACHED.get(name, set()) & reached[name]), (name, sorted(reached[name]))
