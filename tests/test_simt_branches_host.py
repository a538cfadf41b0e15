"""The workgroup records of the two-wave leaf factor form (csrc/sparse_records.cpp: simt_task_segments(), Build_Simt_Branches();
what factor_simt_kernel_branches reads) on the CPU.  tests/simt_branches_driver.cpp is a stand-alone program: compiled with the
host sources csrc/plan.cpp, csrc/host_pool.cpp and csrc/sparse_records.cpp, it builds plan and lane-per-task tables -- with
every two-bin shape split -- of pose chains with loop closures (300 and 612 block columns, d = 6), of the hub graph and of the
"islands" system (a chain plus single poses, pairs and paths of three), each with subtree_size 8 at leaf_size 1 and 3 and at
widths 32 and 16.  For every split task it requires its columns to lie in exactly one segment each, every block or y a column
reads of its own task to have been produced earlier in the same segment or, for the join segment, in either bin, no bin to
read from the other bin or from the joins, and the three segments' lanes to hold the same task; for every stage the records
to cover every chunk exactly once.  It replays the factorization twice in plain C++ -- task by task from the Plan, segment by
segment from the records' programs and tables alone -- and requires equality element for element.  Run plain and with
-fsanitize=address,undefined; nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam_plus_plus_amd", "csrc")

NAMES = {f"{g}-leaf{l}-w{w}" for g in ("chain300", "chain612", "hub", "islands") for l in (1, 3) for w in (32, 16)}
# what the systems together must have reached
REACHED = {"split_two_tips", "split_three_tips", "one_column_bin", "two_column_joins", "whole_task", "odd_whole_chunks",
           "single_whole_chunk", "pair_of_whole_chunks", "spare_lanes"}


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_segments_reproduce_the_task_walk(tmp_path, sanitize):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if not os.path.isfile(os.path.join(rocm, "include", "hip", "hip_runtime.h")):
        pytest.skip("no HIP headers")             # (sparse_kernels.h names longlong2 and hipStream_t)
    exe = tmp_path / "simt_branches_driver"
    flags = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"] if sanitize else []
    cmd = ["g++", "-O1", "-g", "-std=c++17"] + flags + [
        "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"), "-I" + CSRC,
        os.path.join(ROOT, "tests", "simt_branches_driver.cpp"), os.path.join(CSRC, "plan.cpp"),
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
        assert {"split_two_tips", "one_column_bin", "two_column_joins", "spare_lanes"} <= got, (name, sorted(got))
    assert REACHED <= set().union(*reached.values()), sorted(REACHED - set().union(*reached.values()))
