"""The workgroup records of the two-wave leaf backward form (csrc/sparse_records.cpp: Build_Simt_Bwd_Branches(); what
backward_simt_kernel_branches reads) on the CPU.  tests/simt_bwd_branches_driver.cpp is a stand-alone program: compiled with the
host sources csrc/plan.cpp, csrc/host_pool.cpp and csrc/sparse_records.cpp, it builds plan and lane-per-task tables -- with every
two-bin shape split, by the backward form's knob alone -- of the graphs of tests/test_simt_branches_host.py, each with
subtree_size 8 at leaf_size 1 and 3 and at widths 32 and 16.  From the records alone it requires every column of every split
task to lie in exactly one segment, the places the segments carry to be a permutation of the task's columns, every row of a
bin's column inside the task to be a column of the same bin or a join, every segment's table and places to fit the stage's LDS
regions, and the records to cover every chunk once in the factor form's order; it replays the substitution from the Plan and
from the records and requires equal solutions; and it requires the chunk, program and table arrays of the one-wave forms to
be the same bytes with and without the records.  Run plain and with -fsanitize=address,undefined; nothing is loaded into
Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam_plus_plus_amd", "csrc")

NAMES = {f"{g}-leaf{l}-w{w}" for g in ("chain300", "chain612", "hub", "islands") for l in (1, 3) for w in (32, 16)}
# what the systems together must have reached
REACHED = {"split_two_tips", "split_three_tips", "one_join", "two_joins", "segment_column_beyond_the_set", "two_rows_outside",
           "spare_lanes", "split_spare_lanes", "odd_whole_chunks", "single_whole_chunk", "pair_of_whole_chunks"}


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_backward_segments_reproduce_the_task_walk(tmp_path, sanitize):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if not os.path.isfile(os.path.join(rocm, "include", "hip", "hip_runtime.h")):
        pytest.skip("no HIP headers")             # (sparse_kernels.h names longlong2 and hipStream_t)
    exe = tmp_path / "simt_bwd_branches_driver"
    flags = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else []
    cmd = ["g++", "-O1", "-g", "-std=c++17"] + flags + [
        "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + CSRC,
        os.path.join(ROOT, "tests", "simt_bwd_branches_driver.cpp"), os.path.join(CSRC, "plan.cpp"),
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
    assert set(reached) == NAMES, run.stdout
    for name, got in reached.items():
        assert {"split_two_tips", "one_join", "two_joins", "spare_lanes"} <= got, (name, sorted(got))
    assert REACHED <= set().union(*reached.values()), sorted(REACHED - set().union(*reached.values()))
