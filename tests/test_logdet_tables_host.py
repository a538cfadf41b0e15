"""The pivot table of slampp_hip_logdet (csrc/logdet_tables.cpp) on the CPU.  The unit depends on plan.h alone and makes no
device calls, so it is compiled here with g++ -fsanitize=address,undefined together with csrc/plan.cpp and a stand-alone
driver (tests/logdet_tables_driver.cpp).  The driver plans the graphs of tests/driver_graphs.h -- with no dense top, with a
forced one whose chains are aligned to tiles (gaps) and with a packed one -- and checks that every scalar pivot is listed
exactly once, at loff(diagonal block) + i (d + 1) or at its position in the dense top, that there are n_scalars entries and
that none lies in a gap or the padding.  A second test hands the driver the structures of two golden systems and compares
the table it prints with the offsets recomputed here from the plan the library gives Python (hip_solver.host_plan)."""
import os
import re
import shutil
import subprocess

import pytest

from golden_util import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam_plus_plus_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("logdet_tables") / "logdet_tables_driver"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I" + CSRC,
           os.path.join(ROOT, "tests", "logdet_tables_driver.cpp"), os.path.join(CSRC, "plan.cpp"),
           os.path.join(CSRC, "logdet_tables.cpp"), "-o", str(exe), "-lpthread"]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "sanitizer" in (build.stderr or "").lower() and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    return str(exe)


def _run(exe, args=()):
    run = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
    return run.stdout


def test_every_pivot_is_listed_once_and_clean_under_sanitizers(driver):
    lines = _run(driver).splitlines()
    assert len(lines) == 7 and all(l.endswith(" ok") for l in lines), lines
    got = {l.split(":")[0]: [int(x) for x in re.findall(r"(?:pivots|dense|gaps) (\d+)", l)] for l in lines}
    assert got["chain"][0] == 6000 * 6 and got["grid"] == [4800, 0, 0] and got["mixed"][1] == 0
    pivots, dense, gaps = got["grid+dense_top"]
    assert pivots == 4800 and 0 < dense < pivots                         # the forced dense top is there
    pivots, dense, gaps = got["grid7+dense_top"]
    assert pivots == 11200 and 0 < dense < pivots and gaps > 0           # ... and one with alignment gaps
    assert got["grid7+dense_top_packed"] == [pivots, dense, 0]


@pytest.mark.parametrize("name,dense_top_nb", [("chain6_n60", 0), ("sphere_8x8", 2), ("manhattan_n150", -1)])
def test_table_matches_the_plan_python_sees(driver, built, name, dense_top_nb):
    from slam_plus_plus_amd import hip_solver
    lam, _ = load_golden(name)
    plan, _ = hip_solver.host_plan(lam, dense_top_nb=dense_top_nb)
    expected = []
    for j in range(plan["n_bcols"]):
        d = int(plan["dim"][j])
        if plan["dense_dim"] > 0 and plan["dense_pos"][j] >= 0:
            expected += [-(1 + int(plan["dense_pos"][j]) + i) for i in range(d)]
        else:
            loff = int(plan["loff"][plan["lptr"][j]])
            expected += [loff + i * (d + 1) for i in range(d)]
    args = [lam.n_bcols] + lam.cumsum.tolist() + lam.bcol_ptr.tolist() + lam.brow_idx.tolist() + [dense_top_nb]
    out = _run(driver, args)
    assert out.startswith("table:"), out[:200]
    table = [int(x) for x in out.split(":", 1)[1].split()]
    assert len(table) == lam.n_scalars == len(expected)
    assert table == expected and len(set(table)) == len(table)
