"""The backward records of the slice tasks (csrc/sparse_records.cpp: CPanelPass::Append_Backward_Record; what
backward_slice_kernel reads) on the CPU.  tests/backward_records_driver.cpp is a stand-alone program: compiled with the
host sources csrc/plan.cpp, csrc/host_pool.cpp and csrc/sparse_records.cpp, it builds plan and records of pose chains with
loop closures (40, 300 and 612 block columns at d = 3, 6, 7; subtree_size 4, leaf_size 1, no dense top), of the 612-pose
chain with the launch shapes of crowded stages (two and four columns per wave), of a hub graph (a chain plus one vertex
joined to 60 poses: columns with more than nine blocks) and of that hub with a clique hanging off it (tasks over the panel
capacities, left to the column kernel beside packaged ones).  It runs the backward substitution twice in plain C++ --
column by column from the Plan, and level by level from the backward records alone with internal x only from a per-task
array -- and requires the two results equal element for element, every internal x read produced by an earlier level of
the same task, and the packaged tasks and the rest list of a stage to be exactly the stage's tasks.  Run plain and with
-fsanitize=address,undefined; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam_plus_plus_amd", "csrc")

COMMON = {"slice_stages", "multi_level_task", "level_of_several_columns", "internal_x"}
REACHED = {f"chain{d}-{n}": COMMON | {"one_col_per_wave"} for d in (3, 6, 7) for n in (40, 300, 612)}
REACHED["chain6-612-four-waves"] = COMMON | {"two_cols_per_wave"}
REACHED["chain7-612-two-waves"] = COMMON | {"four_cols_per_wave"}
for _d in (3, 6, 7):
    REACHED[f"hub{_d}"] = COMMON | {"column_over_eight_blocks"}      # (eight below the diagonal: more than nine blocks)
    REACHED[f"hub-clique{_d}"] = COMMON | {"column_over_eight_blocks", "rest_tasks"}


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_backward_records_reproduce_the_column_walk(tmp_path, sanitize):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if not os.path.isfile(os.path.join(rocm, "include", "hip", "hip_runtime.h")):
        pytest.skip("no HIP headers")             # (sparse_kernels.h names longlong2 and hipStream_t)
    exe = tmp_path / "backward_records_driver"
    flags = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else []
    cmd = ["g++", "-O1", "-g", "-std=c++17"] + flags + [
        "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + CSRC,
        os.path.join(ROOT, "tests", "backward_records_driver.cpp"), os.path.join(CSRC, "plan.cpp"),
        os.path.join(CSRC, "host_pool.cpp"), os.path.join(CSRC, "sparse_records.cpp"), "-o", str(exe), "-lpthread"]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if sanitize and build.returncode != 0 and "sanitizer" in (build.stderr or "").lower() and "cannot find" in build.stderr:
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
