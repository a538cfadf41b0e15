"""The kernels of the dense top on tile patterns handed to them directly (csrc/dense_tiles.hip: tile_cholesky and
tile_backsolve by CTileSchedule's tables; csrc/dense_chol.hip: dense_cholesky, dense_forwardsolve, dense_backsolve), reached
through oracle/libtile_probe.so: one call factors and solves by the tile schedule, solves a second right-hand side on the kept
factor, factors and solves a fresh copy by the dense schedule, and returns every result and the device tables.

The reference is a Cholesky factor and its solutions computed column by column in numpy.longdouble
(tests/dense_tile_cases.py).  The systems are the diagonally dominant ones of tests/tile_replay.py (entries within +-0.4); for
every case of this file numpy's own fp64 factor of them stays under a tenth of L_TOL from the long-double one (at most 3e-16
relative; tests/test_tile_schedule_host.py::test_numpy_fp64_factor_is_a_tenth_of_the_bound_from_the_reference asserts it on
the CPU), so the project's bounds -- L_TOL on max|L - L_ref| / max|L_ref|, TOL on x -- are bounds on the kernels, not on the
reference.

The patterns are the designed ones of the host test up to 15 tile columns, and full lower triangles with 1, 2, 4, 5, 8, 9, 12,
13, 14 and 15 tile columns: one to four outer panels of the dense schedule (4 tiles each).  Its far update -- panel b - 1
applied to the panels from b + 2 on, so the first one is panel 0 on the tile columns from 12 -- exists from 13 tile columns
on: 1, 2 and 3 trailing tile columns at 13, 14 and 15."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import dense_tile_cases as D
import tile_replay as R
from variant_util import L_TOL, TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam_plus_plus_amd", "csrc")
NB = R.NB
PATTERNS, case = D.PATTERNS, D.case
DEFAULT, KNOBS = (4, 1024), [(1, 1), (64, 1)]
TABLE_KEYS = ["potrf", "trsm", "tgt", "src", "riders", "back_diag", "back_carry", "level_potrf_ptr", "level_trsm_ptr",
              "level_tgt_ptr", "level_urgent_end", "rider_ptr", "back_diag_ptr", "back_carry_ptr"]


# ---- the probe ----

@functools.lru_cache(maxsize=None)
def probe_lib():
    lib = C.CDLL(os.path.join(ROOT, "oracle", "libtile_probe.so"))  # (built by oracle/Makefile; a missing library is an error)
    lib.tile_probe_run.restype = C.c_int
    lib.tile_probe_run.argtypes = [C.c_int, C.c_char_p, C.c_int] + [C.c_void_p] * 8 + [C.c_int]
    return lib


def probe(nz, n, M, b2):
    """one call of the probe: dict of L_tile, L_dense, x_tile, x_again, x_dense, the two flags, Build's answer, the tables"""
    T = nz.shape[0]
    n_pad = T * NB
    assert M.shape == (n_pad, n_pad) and 1 <= n <= n_pad - 1
    flags = np.ascontiguousarray(np.asarray(nz, dtype=np.int8).flatten(order="F"))
    M_in = np.asfortranarray(M, dtype=np.float64)
    L_tile, L_dense = np.zeros((n_pad, n_pad), order="F"), np.zeros((n_pad, n_pad), order="F")
    x = np.zeros(3 * n_pad)
    status, sizes = np.zeros(4, dtype=np.int32), np.zeros(14, dtype=np.int32)
    tables = np.zeros(16 * T * T * T + 64 * T + 64, dtype=np.int32)  # (a target per tile, at most T sources each, twice over)
    b2 = np.ascontiguousarray(b2, dtype=np.float64)
    rc = probe_lib().tile_probe_run(T, flags.tobytes(), n, M_in.ctypes.data, b2.ctypes.data, L_tile.ctypes.data, L_dense.ctypes.data,
                                    x.ctypes.data, status.ctypes.data, sizes.ctypes.data, tables.ctypes.data, len(tables))
    assert rc == 0, "tile_probe_run: %d" % rc
    out = {"L_tile": L_tile, "L_dense": L_dense, "x_tile": x[:n], "x_again": x[n_pad:n_pad + n], "x_dense": x[2 * n_pad:2 * n_pad + n],
           "flag_tile": int(status[0]), "flag_dense": int(status[1]), "built": bool(status[2]), "n_levels": int(status[3])}
    at = 0
    for key, size in zip(TABLE_KEYS, sizes):
        v = tables[at:at + size].copy()
        out[key] = v.reshape(-1, 4) if key in ("trsm", "tgt", "riders", "back_diag", "back_carry") else v
        at += size
    return out


@pytest.fixture(scope="module")
def host_tables(tmp_path_factory):
    """what the host function gives for every pattern and knob setting of this module: {(name, knobs): tables}"""
    assert shutil.which("g++") is not None, "g++ builds tests/tile_schedule_driver.cpp: a missing compiler is an error"
    d = tmp_path_factory.mktemp("tile_tables")
    exe = d / "tile_schedule_driver"
    build = subprocess.run(["g++", "-O1", "-std=c++17", "-I" + CSRC, os.path.join(ROOT, "tests", "tile_schedule_driver.cpp"),
                            os.path.join(CSRC, "tile_schedule.cpp"), os.path.join(CSRC, "plan.cpp"), "-o", str(exe), "-lpthread"],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-2000:]
    keys = [(name, knobs) for name in PATTERNS for knobs in [DEFAULT] + KNOBS]
    (d / "cases.txt").write_text("".join(R.pattern_text(PATTERNS[name], *knobs) for name, knobs in keys))
    run = subprocess.run([str(exe), str(d / "cases.txt")], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    cases = R.parse_driver_output(run.stdout)
    assert len(cases) == len(keys)
    return dict(zip(keys, cases))


def set_knobs(monkeypatch, knobs=None, wide_min_tiles=None):
    """the development knobs of the two schedules; the switch that lets the library read them is itself read where a handle is
    created (csrc/plan.h), so one is created"""
    from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP
    monkeypatch.setenv("SLAMPP_HIP_DEV", "1")
    for key, value in (("SLAMPP_HIP_DEV_RIDER_CHUNK", knobs and knobs[0]), ("SLAMPP_HIP_DEV_RIDER_BUDGET", knobs and knobs[1]),
                       ("SLAMPP_HIP_DEV_WIDE_MIN_TILES", wide_min_tiles)):
        if value is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, str(value))
    CLinearSolver_HIP(device=0)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def check_against_reference(c, r, label, M=None, tile_only=False):
    """the bounds of the module's docstring on one probe result of the matrix M (the case's own unless given); tile_only: what
    tile_cholesky and the first tile_backsolve gave, nothing else"""
    n, mask, dense = c["n"], c["mask"], not tile_only
    scale = float(np.abs(c["L_ref"]).max())
    lower = np.tril(np.ones((n, n), dtype=bool))
    ref = np.asarray(c["L_ref"], dtype=np.float64)
    err_L = {"tile": float(np.abs((r["L_tile"][:n, :n] - ref)[lower & mask[:n, :n]]).max() / scale)}
    err_x = {"tile": R_rel(r["x_tile"], c["x_ref"])}
    if dense:
        err_x["again"] = R_rel(r["x_again"], c["x2_ref"])
        err_L["dense"] = float(np.abs((r["L_dense"][:n, :n] - ref)[lower]).max() / scale)
        err_x["dense"] = R_rel(r["x_dense"], c["x_ref"])
        err_x["tile against dense"] = R_rel(r["x_tile"], r["x_dense"])
    print("%s: L %s; x %s" % (label, ", ".join("%s %.2e" % kv for kv in err_L.items()), ", ".join("%s %.2e" % kv for kv in err_x.items())))
    assert r["built"] and r["flag_tile"] == 0 and (not dense or r["flag_dense"] == 0), label
    assert all(v < L_TOL for v in err_L.values()), (label, err_L)
    assert all(v < (1e-11 if k == "tile against dense" else TOL) for k, v in err_x.items()), (label, err_x)
    # tiles outside the filled pattern (the upper triangle's as well): the bits they had
    assert np.array_equal(bits(r["L_tile"])[~(mask | mask.T)], bits(c["M"] if M is None else M)[~(mask | mask.T)]), label


def R_rel(x, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(x - ref).max() / np.abs(ref).max())


def check_tables(r, host, label):
    assert host["ok"] and r["n_levels"] == host["n_levels"], label
    for key in TABLE_KEYS:
        assert r[key].dtype == host[key].dtype and r[key].tobytes() == host[key].tobytes(), (label, key, r[key], host[key])


# ---- the tests ----

@pytest.mark.parametrize("knobs", [None] + KNOBS, ids=["default", "chunk1_budget1", "chunk64_budget1"])
@pytest.mark.parametrize("name", list(PATTERNS))
def test_both_schedules_against_longdouble(monkeypatch, name, knobs):
    """factor, the three solutions and the untouched tiles; the same call twice gives the same bits"""
    c = case(name)
    set_knobs(monkeypatch, knobs)
    r = probe(c["nz"], c["n"], c["M"], c["b2"])
    label = "%s (T = %d, n = %d), knobs %s" % (name, c["nz"].shape[0], c["n"], knobs or "default")
    check_against_reference(c, r, label)
    again = probe(c["nz"], c["n"], c["M"], c["b2"])
    for key in ("L_tile", "L_dense", "x_tile", "x_again", "x_dense"):
        assert np.array_equal(bits(r[key]), bits(again[key])), (label, key)


@pytest.mark.parametrize("knobs", [None] + KNOBS, ids=["default", "chunk1_budget1", "chunk64_budget1"])
@pytest.mark.parametrize("name", list(PATTERNS))
def test_device_tables_are_the_host_functions(monkeypatch, host_tables, name, knobs):
    """Build returned true, and what it uploaded is what tile_schedule_tables gives for the pattern and the knobs, byte for
    byte; the device's tables also pass the CPU replay"""
    c = case(name)
    set_knobs(monkeypatch, knobs)
    r = probe(c["nz"], c["n"], c["M"], c["b2"])
    label = "%s, knobs %s" % (name, knobs or "default")
    assert r["built"], label
    check_tables(r, host_tables[(name, knobs or DEFAULT)], label)
    R.replay_symbolic(c["nz"], dict(r, ok=True, height=R.fill(c["nz"])[1]), *(knobs or DEFAULT))


@pytest.mark.parametrize("name", ["full12", "full13", "full14", "full15"])
def test_dense_schedule_with_wide_far_updates(monkeypatch, name):
    """SLAMPP_HIP_DEV_WIDE_MIN_TILES=2 puts a far update of at least two trailing tile columns on the 128 x 128 jobs.  With 4
    tiles per outer panel the far update of these sizes is panel 0 on the tile columns from 12: none at 12 tile columns and
    one column at 13 (the knob changes nothing there: 64 x 64 jobs or none), two at 14 (an even number: all of it on one
    128 x 128 job) and three at 15 (odd: the first of them stays with the 64 x 64 jobs)."""
    c = case(name)
    n_far = max(c["nz"].shape[0] - 3 * 4, 0)
    assert n_far == {"full12": 0, "full13": 1, "full14": 2, "full15": 3}[name]
    set_knobs(monkeypatch, None, wide_min_tiles=2)
    r = probe(c["nz"], c["n"], c["M"], c["b2"])
    check_against_reference(c, r, "%s, wide far updates" % name)
    set_knobs(monkeypatch, None)
    same = np.array_equal(bits(r["L_dense"]), bits(probe(c["nz"], c["n"], c["M"], c["b2"])["L_dense"]))
    print("%s: the knob %s the bits of the dense factor" % (name, "keeps" if same else "changes"))
    assert same or n_far >= 2, name   # (below two trailing tile columns the launches are the same ones)


@pytest.mark.parametrize("n_short", [1, 64, 65], ids=["n_pad-1", "n_pad-64", "n_pad-65"])
@pytest.mark.parametrize("name", ["fill6", "meet3", "tree15"])
def test_edges_of_n_with_nan_outside_the_pattern(monkeypatch, name, n_short):
    """n at the edges of the padded size, and every tile outside the filled pattern NaN: the tile schedule reads none of them.
    (The dense schedule and dense_forwardsolve read the whole lower triangle by design: their results are not looked at here.)"""
    c = case(name, n_short)
    set_knobs(monkeypatch, None)
    outside = ~(c["mask"] | c["mask"].T)
    M = np.array(c["M"], order="F")
    M[outside] = np.nan
    r = probe(c["nz"], c["n"], M, c["b2"])
    n = c["n"]
    assert np.isfinite(r["x_tile"]).all() and np.isfinite(np.tril(r["L_tile"][:n, :n])[c["mask"][:n, :n]]).all()
    check_against_reference(c, r, "%s, n = n_pad - %d = %d, NaN outside" % (name, n_short, n), M=M, tile_only=True)


def test_not_positive_definite_raises_the_flag_in_both_schedules(monkeypatch):
    c = case("chain8", 5)
    set_knobs(monkeypatch, None)
    assert R.fill(c["nz"])[1][2] == 2                           # a tile column of height 2
    n = c["n"]
    for row, want in ((2 * NB + 5, 1), (n + 1, 0)):              # a row of the system; a row of the padding
        M = np.array(c["M"], order="F")
        M[row, row] = -1.0
        r = probe(c["nz"], n, M, c["b2"])
        assert r["built"] and (r["flag_tile"] & 1, r["flag_dense"] & 1) == (want, want), (row, r["flag_tile"], r["flag_dense"])


@pytest.mark.parametrize("tiles", [1, 0])
def test_dense_top_tiles_option_selects_the_schedule(monkeypatch, capfd, tiles):
    """the option's wiring: the analysis says which schedule the dense top took"""
    from golden_util import load_golden
    from oracle import oracle_lib as O
    from slam_plus_plus_amd.hip_solver import CLinearSolver_HIP
    lam = load_golden("manhattan_n150")[0]
    ok, x_ref, _ = O.solve_sparse(lam)
    monkeypatch.setenv("SLAMPP_HIP_PLAN_TIMING", "1")
    solver = CLinearSolver_HIP(dense_top_nb=2, dense_top_min_dim=0, dense_top_tiles=tiles)
    capfd.readouterr()
    eta = lam.rhs.copy()
    assert ok and solver.Solve_PosDef(lam, eta)
    err = capfd.readouterr().err
    lines = [l for l in err.splitlines() if l.startswith("[setup] dense top:")]
    assert len(lines) == 1 and lines[0].endswith("-> %s schedule" % ("tile" if tiles else "dense")), err[-2000:]
    assert R_rel(eta, x_ref) < TOL
