"""The tables of the dense top's tile schedule (csrc/tile_schedule.cpp) on the CPU: a stand-alone driver
(tests/tile_schedule_driver.cpp, compiled here with g++) writes them out for patterns handed to it directly, and
tests/tile_replay.py replays them launch by launch -- symbolically (every hazard a deterministic failure) and with numpy tile
operations against numpy's dense Cholesky.  The patterns: a designed set at four settings of the rider knobs, 300 seeded
random ones with 1 to 40 tile columns, and the planner's own for a sphere and a Manhattan world.  The same program is also
built with -fsanitize=address,undefined and has to write the same tables."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import dense_tile_cases as D
import tile_replay as R
from variant_util import L_TOL, TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam_plus_plus_amd", "csrc")
DESIGNED = R.designed_patterns()
N_RANDOM = 300


def _random_cases():
    rng = np.random.default_rng(20240611)
    return [(R.random_pattern(rng), R.KNOBS[int(rng.integers(len(R.KNOBS)))] if rng.random() < 0.7 else
             (int(rng.integers(1, 9)), int(rng.integers(1, 40)))) for _ in range(N_RANDOM)]


def _graph_text(lam, chunk, budget):
    nums = np.concatenate([np.asarray(lam.cumsum, dtype=np.int64), np.asarray(lam.bcol_ptr, dtype=np.int64),
                           np.asarray(lam.brow_idx, dtype=np.int64)])
    return "graph %d %d %d %d %s\n" % (len(lam.cumsum) - 1, len(lam.brow_idx), chunk, budget, " ".join(str(v) for v in nums))


def _build_driver(path, sanitize):
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-I" + CSRC, os.path.join(ROOT, "tests", "tile_schedule_driver.cpp"),
           os.path.join(CSRC, "tile_schedule.cpp"), os.path.join(CSRC, "plan.cpp"), "-o", str(path), "-lpthread"]
    if sanitize:
        cmd[1:1] = ["-fsanitize=" + sanitize, "-fno-omit-frame-pointer"]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "sanitizer" in (build.stderr or "").lower() and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]


def _run_driver(exe, path):
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert run.returncode == 0, (run.stdout[-500:] + run.stderr)[-3000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    return run.stdout


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """one run of the plain driver over every case of this module: {"designed": {(name, knobs): tables}, "random": [...],
    "graphs": {name: tables}, "exe": ..., "input": ..., "stdout": ...}"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    from slam_plus_plus_amd import synth
    d = tmp_path_factory.mktemp("tile_schedule")
    keys, text = [], []
    for name, nz in DESIGNED.items():
        for knobs in R.KNOBS:
            keys.append(("designed", (name, knobs), nz, knobs))
            text.append(R.pattern_text(nz, *knobs))
    for n, (nz, knobs) in enumerate(_random_cases()):
        keys.append(("random", n, nz, knobs))
        text.append(R.pattern_text(nz, *knobs))
    for name, lam in (("sphere", synth.sphere(40, 40, seed=5)), ("manhattan", synth.manhattan(3000, seed=6))):
        keys.append(("graphs", name, None, R.KNOBS[0]))
        text.append(_graph_text(lam, *R.KNOBS[0]))
    path = d / "cases.txt"
    path.write_text("".join(text))
    exe = d / "tile_schedule_driver"
    _build_driver(exe, "")
    stdout = _run_driver(exe, path)
    cases = R.parse_driver_output(stdout)
    assert len(cases) == len(keys)
    out = {"designed": {}, "random": {}, "graphs": {}, "input": path, "stdout": stdout, "dir": d}
    for (kind, key, nz, knobs), t in zip(keys, cases):
        assert (t["chunk"], t["budget"]) == knobs and (nz is None or np.array_equal(np.tril(nz), np.tril(t["nz"])))
        out[kind][key] = t
    return out


@pytest.mark.parametrize("knobs", R.KNOBS, ids=lambda k: "chunk%d_budget%d" % k)
@pytest.mark.parametrize("name", list(DESIGNED))
def test_designed_pattern_replays(tables, name, knobs):
    t = tables["designed"][(name, knobs)]
    R.replay_symbolic(DESIGNED[name], t, *knobs)
    err_L, err_x = R.replay_numeric(DESIGNED[name], t, seed=3, n=DESIGNED[name].shape[0] * R.NB - 3)
    print(f"{name} {knobs}: L {err_L:.2e}, x {err_x:.2e}")
    assert err_L < L_TOL and err_x < TOL, (err_L, err_x)


def test_random_patterns_replay(tables):
    cases = _random_cases()
    for n, (nz, knobs) in enumerate(cases):
        try:
            R.replay_symbolic(nz, tables["random"][n], *knobs)
        except R.ReplayError as e:
            raise AssertionError("random pattern %d (T = %d, knobs %s): %s" % (n, nz.shape[0], knobs, e))
    small = [n for n, (nz, _) in enumerate(cases) if 2 <= nz.shape[0] <= 10][:12]
    assert len(small) == 12
    for n in small:
        err_L, err_x = R.replay_numeric(cases[n][0], tables["random"][n], seed=n)
        assert err_L < L_TOL and err_x < TOL, (n, err_L, err_x)


@pytest.mark.parametrize("name", ["sphere", "manhattan"])
def test_planner_patterns_replay(tables, name):
    t = tables["graphs"][name]
    assert t["T"] >= 2
    R.replay_symbolic(t["nz"], t, *R.KNOBS[0])


def test_designed_set_reaches_every_form(tables):
    """a case set that does not reach a form of the schedule proves nothing about it"""
    reach = set()
    for (name, knobs), t in tables["designed"].items():
        reach |= R.replay_symbolic(DESIGNED[name], t, *knobs)
    assert not [r for r in R.REACH if r not in reach], sorted(reach)


def _broken(t, **changes):
    out = dict(t)
    for key, fn in changes.items():
        out[key] = t[key].copy()
        fn(out[key])
    return out


def test_replay_rejects_broken_tables(tables):
    """the replay on tables spoilt by hand: each must be refused"""
    nz, knobs = DESIGNED["full6"], R.KNOBS[0]
    t = tables["designed"][("full6", knobs)]
    R.replay_symbolic(nz, t, *knobs)

    def flip_carry_flag(v): v[1, 2] ^= 1
    def flip_diag_flag(v): v[-1, 2] ^= 1
    def second_z(v): v[1, 2] = 1                       # (2, 0) also updates its diagonal tile
    def drop_source(v): v[-1] = v[-3]                  # (5, 5) takes column 2 twice and column 3 never
    def swap_levels(v): v[[0, 1]] = v[[1, 0]]          # column 1 factored in the first launch
    def early_rider(v): v[1] = v[2]                    # the second launch's riders take the third's along
    for change in ({"back_carry": flip_carry_flag}, {"back_diag": flip_diag_flag}, {"trsm": second_z}, {"src": drop_source},
                   {"potrf": swap_levels}, {"rider_ptr": early_rider}):
        with pytest.raises(R.ReplayError):
            R.replay_symbolic(nz, _broken(t, **change), *knobs)


@pytest.mark.parametrize("flags", ["", "address,undefined"], ids=["plain", "sanitized"])
def test_driver_writes_the_same_tables(tables, flags):
    """the same program again, and built with AddressSanitizer + UBSan: a clean run and the same tables"""
    exe = tables["dir"] / ("tile_schedule_driver_" + (flags.replace(",", "_") or "again"))
    _build_driver(exe, flags)
    assert _run_driver(exe, tables["input"]) == tables["stdout"]


@pytest.mark.parametrize("name,n_short", D.all_cases(), ids=lambda v: str(v))
def test_numpy_fp64_factor_is_a_tenth_of_the_bound_from_the_reference(name, n_short):
    """every system of tests/test_dense_tiles_gpu.py: its long-double reference is not what the bounds there measure"""
    c = D.case(name, n_short)
    err = float(np.abs(np.linalg.cholesky(c["A"]) - c["L_ref"]).max() / np.abs(c["L_ref"]).max())
    assert err < 0.1 * L_TOL, (name, n_short, err)
