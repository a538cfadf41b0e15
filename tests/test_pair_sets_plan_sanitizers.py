"""The host planning of covariance blocks at pairs of column sets under sanitizers (CPU only).  plan_pair_sets
(csrc/pair_plan.cpp) plans pairs of columns that are sets of source block columns with a scalar width -- the camera and
landmark columns of a BA system over its reduced camera system.  It is compiled here with g++ -fsanitize=address,undefined
together with csrc/plan.cpp and a stand-alone driver (tests/pair_sets_plan_driver.cpp) that plans a band, a band with a
forced dense top, a star and a graph of two components, and checks seeded lists of multi-source pairs against a brute-force
union and intersection of the paths in parent[]: every pass has at most 48 scalar columns, holds both columns of each of
its pairs at the lanes recorded and lists each source once, the passes are greedy, each pair's row list is exactly the
intersection of the two reaches in schedule order, the dense flag is right, and sets of one source each reproduce
plan_pairs record for record."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam_plus_plus_amd", "csrc")


def test_pair_set_planner_is_right_and_clean_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "pair_sets_plan_driver"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I" + CSRC,
           os.path.join(ROOT, "tests", "pair_sets_plan_driver.cpp"), os.path.join(CSRC, "plan.cpp"),
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
    assert len(lines) == 20 and all(l.endswith(" ok") for l in lines), run.stdout      # four graphs: four lists + plan_pairs
    dense = [int(re.search(r"dense_dim (\d+)", l).group(1)) for l in lines if l.startswith("band+dense_top: pairs")]
    assert len(dense) == 4 and all(d > 0 for d in dense), run.stdout                   # the forced dense top is there
    passes = [int(re.search(r"passes (\d+)", l).group(1)) for l in lines]
    assert max(passes) > 2, run.stdout                                                 # several passes were planned
