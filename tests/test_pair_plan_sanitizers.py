"""The host planning of covariance blocks at arbitrary pairs under sanitizers (CPU only).  csrc/pair_plan.cpp depends on
plan.h alone and makes no device calls, so it is compiled here with g++ -fsanitize=address,undefined together with
csrc/plan.cpp and a stand-alone driver (tests/pair_plan_driver.cpp) that plans a chain with loop closures, a chain of mixed
block sizes, a grid with and without a forced dense top and a graph in several pieces, and checks seeded pair lists
against a brute-force walk of parent[]: every pass has at most 48 scalar columns and holds both columns of each of its
pairs, each pair's row list is exactly the intersection of the two paths in schedule order, the dense flag is right, and
every pair is planned once."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam_plus_plus_amd", "csrc")


def test_pair_planner_is_right_and_clean_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "pair_plan_driver"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I" + CSRC,
           os.path.join(ROOT, "tests", "pair_plan_driver.cpp"), os.path.join(CSRC, "plan.cpp"),
           os.path.join(CSRC, "pair_plan.cpp"), "-o", str(exe), "-lpthread"]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "sanitizer" in (build.stderr or "").lower() and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == 20 and all(l.endswith(" ok") for l in lines), run.stdout      # five graphs, four pair lists each
    dense = [int(re.search(r"dense_dim (\d+)", l).group(1)) for l in lines if l.startswith("grid+dense_top:")]
    assert len(dense) == 4 and all(d > 0 for d in dense), run.stdout                   # the forced dense top is there
    passes = [int(re.search(r"passes (\d+)", l).group(1)) for l in lines]
    assert max(passes) > 1, run.stdout                                                 # more than one pass was planned
