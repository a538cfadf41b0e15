"""The host builder of the Lambda / eta assembly under sanitizers (CPU only).  csrc/assembly_tables.cpp makes no device call
and includes nothing of ROCm, so it is compiled here with plain g++ -fsanitize=address,undefined together with a stand-alone
driver (tests/assembly_tables_driver.cpp) and run directly.  The driver reads the designed cases of tests/assembly_cases.py,
runs the builder and decodes every table the way the kernel that reads it does, against a brute-force walk of the edges:
every block of Lambda (edge-less ones included) written by exactly one record of exactly one kernel family and every
vertex's eta once; every (edge, block, flip / side) exactly once in its record's list, in edge order, a single entry in the
record itself; the group packages' header counts, slots, padding, field widths, item order and codes, words and stride;
grouped vertices within the cap, groups closed for a reason, one dimension for the long vertices, the packed vertices small
enough, the maxima.  It names the branches each case reached; a case that does not reach the branches listed for it in
assembly_cases.py fails, and so does one whose anchored vertex takes another route than the case says.  Also: what the builder
must refuse, the sweep of asm_group_shape() that DESIGN.md quotes, and the error of the cases' own reference."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import assembly_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam_plus_plus_amd", "csrc")
ROUTE = {"G": "group", "L": "long", "S": "small", "P": "plain"}

# every branch the issue of these tests names, somewhere among the cases
NAMED = {"group_closed_at_vertex_count", "group_closed_at_edge_cap", "group_closed_at_package_words", "vertex_over_cap_closes_group",
         "no_groups_cap_under_8", "groups_off", "long", "long_dim_taken", "small_packed", "plain_diag", "offdiag_packed",
         "offdiag_plain", "single_entry_record", "edgeless_block", "edgeless_vertex", "multi_edge_block", "flipped_edge",
         "empty_group_package", "group_kernel_0", "group_kernel_2", "group_kernel_3", "group_kernel_6"}


def build_driver(directory, sanitize=True):
    """Compiles the driver (None where there is no g++ or no sanitizer runtime)."""
    if shutil.which("g++") is None:
        return None
    exe = os.path.join(str(directory), "assembly_tables_driver")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-I" + CSRC, os.path.join(ROOT, "tests", "assembly_tables_driver.cpp"),
           os.path.join(CSRC, "assembly_tables.cpp"), "-o", exe]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if build.returncode != 0 and "sanitizer" in (build.stderr or "").lower() and "cannot find" in build.stderr:
        return None
    assert build.returncode == 0, build.stderr[-2000:]
    return exe


def run_driver(exe, args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("SLAMPP_HIP")}
    run = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600,
                         env=dict(env, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    return run.stdout.splitlines()


def parse_case_line(line):
    """name -> (info dict, routes string, reached set) of one line of the driver."""
    name, rest = line.split(": info ", 1)
    info_text, rest = rest.split(" routes ", 1)
    routes, rest = rest.split(" reached", 1)
    info = {k: int(v) for k, v in (t.split("=") for t in info_text.split())}
    return name, info, routes, set(rest.split()[:-1])


def run_cases(exe, cases, directory):
    path = os.path.join(str(directory), "assembly_cases.txt")
    with open(path, "w") as f:
        f.write("".join(A.case_text(c) for c in cases))
    lines = run_driver(exe, [path])
    assert all(l.endswith(" ok") for l in lines), "\n".join(l for l in lines if not l.endswith(" ok"))[-3000:]
    return {p[0]: p[1:] for p in map(parse_case_line, lines)}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = build_driver(tmp_path_factory.mktemp("assembly_tables"))
    if exe is None:
        pytest.skip("no g++ or no sanitizer runtime")
    return exe


def test_tables_are_right_and_clean_under_sanitizers(driver, tmp_path):
    got = run_cases(driver, A.CASES, tmp_path)
    assert set(got) == set(A.BY_NAME)
    everything = set()
    for case in A.CASES:
        info, routes, reached = got[case.name]
        assert case.reached <= reached, (case.name, sorted(case.reached - reached))
        assert not (case.not_reached & reached), (case.name, sorted(case.not_reached & reached))
        assert ROUTE[routes[case.anchor]] == case.anchor_route, (case.name, routes[case.anchor])
        everything |= case.reached
    assert NAMED <= everything, sorted(NAMED - everything)
    assert {c.anchor_route for c in A.CASES} == {"group", "long", "small", "plain"}


def test_builder_refusals(driver):
    lines = run_driver(driver, ["refusals"])
    assert all(l.endswith(" ok") for l in lines), lines
    kinds = {l.split(":")[0].split()[1]: l.split(":")[1].split()[0] for l in lines}
    assert kinds == {"vertex-outside": "invalid_argument", "vertex-negative": "invalid_argument", "self-edge": "invalid_argument",
                     "missing-block": "invalid_argument", "missing-diagonal": "invalid_argument", "dimension-8": "domain_error",
                     "isolated-dimension-8": "domain_error", "rd-0": "invalid_argument", "rd-9": "invalid_argument",
                     "unequal-dimensions": "domain_error", "no-edges": "invalid_argument", "null-vertices": "invalid_argument"}


def test_group_kernel_instantiations_that_can_be_reached(driver):
    """What DESIGN.md section 4.8a says of assemble_group_kernel<RD, *>: 2, 3, 6 and the generic one are reached, 7 by no shape."""
    lines = [l.split() for l in run_driver(driver, ["sweep"])]
    shapes = {l[1]: int(l[3].split("=")[1]) for l in lines if l[1].startswith("RD=")}
    assert shapes == {"RD=2": 49, "RD=3": 49, "RD=6": 49, "RD=7": 0, "RD=0": 107}
    per_rd = {int(l[1].split("=")[1]): int(l[2].split("=")[1]) for l in lines if l[1].startswith("rd=")}
    assert per_rd == {1: 49, 2: 49, 3: 49, 4: 43, 5: 15, 6: 49, 7: 0, 8: 0}
    # the cases' dimensions for the generic kernel and for "no groups" are what the sweep says of them
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        assert "assemble_group_kernel<7, *> is unreachable" in f.read()


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.name)
def test_reference_error_is_under_half_the_bound(case):
    """The bound is one on the kernels, not on the reference: plain fp64 numpy, summed in another order than any kernel does,
    stays under half of it on every entry of every case, with and without the weights and the anchor."""
    lam, es = case.structure(), case.edge_set()
    for weights, unary in ((True, True), (False, False)):
        ref_v, ref_e, _, _, bound_v, bound_e, _, _ = A.reference(lam, es, weights, unary)
        v64, e64 = A.fp64_restatement(lam, es, weights, unary)
        assert np.all(np.abs((v64 - ref_v).astype(np.float64)) <= 0.5 * bound_v)
        assert np.all(np.abs((e64 - ref_e).astype(np.float64)) <= 0.5 * bound_e)
        assert np.all(bound_v[ref_v != 0] > 0) and np.all(bound_e[ref_e != 0] > 0)


def test_reference_layout_against_a_dense_walk():
    """The reference's own indexing, checked on the smallest mixed case element by element against explicit matrices."""
    case = A.BY_NAME["one-edge-flipped"]
    lam, es = case.structure(), case.edge_set()
    ref_v, ref_e = A.reference(lam, es, True, False)[:2]
    J0 = es.J0[0].T.astype(A.LD)                  # rd x d0
    J1 = es.J1[0].T.astype(A.LD)
    S = es.sigma_inv[0].T.astype(A.LD)
    w = A.LD(es.weight[0])
    a, b = int(es.v0[0]), int(es.v1[0])
    assert a > b
    dense = np.zeros((lam.n_scalars, lam.n_scalars), dtype=A.LD)
    cs = lam.cumsum
    dense[cs[b]:cs[b + 1], cs[a]:cs[a + 1]] = (w * (J0.T @ S @ J1)).T
    dense[cs[a]:cs[a + 1], cs[a]:cs[a + 1]] = w * (J0.T @ S @ J0)
    dense[cs[b]:cs[b + 1], cs[b]:cs[b + 1]] = w * (J1.T @ S @ J1)
    off = lam.block_value_offsets()
    for c in range(len(cs) - 1):
        for k in range(int(lam.bcol_ptr[c]), int(lam.bcol_ptr[c + 1])):
            r = int(lam.brow_idx[k])
            blk = dense[cs[r]:cs[r + 1], cs[c]:cs[c + 1]]
            assert np.allclose((ref_v[off[k]:off[k + 1]]).astype(np.float64), blk.T.reshape(-1).astype(np.float64), rtol=1e-15, atol=0)
    eta = np.zeros(lam.n_scalars, dtype=A.LD)
    eta[cs[a]:cs[a + 1]] = w * w * (J0.T @ S @ es.err[0].astype(A.LD))
    eta[cs[b]:cs[b + 1]] = w * (J1.T @ S @ es.err[0].astype(A.LD))
    assert np.allclose(ref_e.astype(np.float64), eta.astype(np.float64), rtol=1e-15, atol=0)
