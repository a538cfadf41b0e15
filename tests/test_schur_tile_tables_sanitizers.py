"""The host builders of the BA analysis under sanitizers (CPU only).  csrc/schur_tile_tables.cpp depends on plan.h,
host_pool.h and host_threads.h alone and makes no device calls, so it is compiled here with plain g++ (no ROCm include
path) -fsanitize=address,undefined together with csrc/host_pool.cpp and a stand-alone driver
(tests/schur_tile_tables_driver.cpp).  The driver builds BA structures, runs the builders in the analysis' order -- the
blocks of S from the bitmap, the routes, the run records, the tile tables and reduce lists, the x-lists, or the full
contribution lists by counting or by comparison sort -- and decodes every table against a brute-force walk of the
landmarks' camera lists: every landmark on exactly one route and the counts right; every (landmark, camera pair) delivered
exactly once to its block of S by a run job (in the kernel's numbering of its partial blocks), a tile slot or an x-list
entry; the run jobs' ranges, prefixes, lengths, reach counts, prefix flags, piece lengths, masking-launch folding and
records; the tiles' limits and launch counts; the reduce lists; the order of the x-lists and of the full lists of both
branches.  The tables must be byte-identical between SLAMPP_HIP_DEV_EMIT_THREADS=1 and 8, between
SLAMPP_HIP_DEV_HOST_THREAD_GRAIN=256 and unset, and between SLAMPP_HIP_DEV_RUN_HASH_ONLY and list comparison; with
SLAMPP_HIP_DEV_NO_PREFIX_RUNS the coverage checks hold.  The driver names the branches each case reached; a case that
does not reach the branches listed for it here fails.  A second build with -fsanitize=thread runs the many-worker cases.

Not reached: rule partial_block_count, which needs 2^31 partial blocks."""
import os
import platform
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam_plus_plus_amd", "csrc")

MIXED = {"runs", "prefix_runs", "masking_launch", "xlists", "over_tile_max_k", "unobserved"}
THREAD_CASES = {
    "mixed-40-many-workers": MIXED | {"many_workers", "tiles", "second_observation_block", "long_track_on_lists"},
    "mixed-40-hashes-alone": MIXED | {"many_workers", "hashes_alone", "tiles"},
    "mixed-40-no-prefix-runs": {"many_workers", "runs", "tiles", "xlists"},
    "random-many-workers": {"many_workers", "rule_runs_impossible", "counting_sort_lists"},
}
REACHED = dict(THREAD_CASES)
REACHED.update({
    "runs-4-64-65-129": {"runs", "pieces_of_32"},
    "runs-piece-mult-2": {"runs"},
    "prefix-chains": {"runs", "prefix_runs", "masking_launch", "second_observation_block"},
    "long-tracks": {"runs", "second_observation_block", "long_track_on_lists", "xlists"},
    "tile-limits": {"tiles", "tile_closed_at_64_blocks", "tile_closed_at_64_points", "over_tile_max_k", "unobserved", "xlists"},
    "rule-runs-impossible": {"rule_runs_impossible", "counting_sort_lists"},
    "rule-no-jobs": {"rule_no_jobs", "counting_sort_lists"},
    "rule-under-half": {"rule_under_half", "counting_sort_lists"},
    "mode-0": {"rule_off", "counting_sort_lists"},
    "rule-sample": {"rule_sample", "counting_sort_lists"},
    "hashes-alone-by-size": {"hashes_alone", "runs"},
    "cameras-70000": {"tile_order_from_lists", "block_of_by_bisection", "comparison_sort_lists", "runs", "tiles", "xlists"},
    "cameras-8200": {"comparison_sort_lists", "block_of_by_bisection", "runs", "tiles", "xlists"},
    "cameras-4100": {"block_of_by_bisection", "runs", "tiles", "xlists"},
})
for _shape in ("6x3", "7x3", "3x2"):
    REACHED["mixed-mode-1-" + _shape] = set(MIXED)
    REACHED["mixed-mode1-" + _shape] = MIXED | {"tiles"}
    REACHED["mixed-mode2-" + _shape] = {"tiles", "xlists", "over_tile_max_k", "unobserved"}
    REACHED["mixed-mode3-" + _shape] = {"runs", "prefix_runs", "masking_launch", "xlists", "unobserved"}
REACHED["mixed-mode-1-6x3"] = MIXED | {"tiles", "long_track_on_lists"}
NOT_REACHED = {"mixed-40-no-prefix-runs": {"prefix_runs", "masking_launch"}, "cameras-4100": {"comparison_sort_lists"},
               "cameras-8200": {"tile_order_from_lists"}}
for _shape in ("6x3", "7x3", "3x2"):
    NOT_REACHED["mixed-mode2-" + _shape] = {"runs"}
    NOT_REACHED["mixed-mode3-" + _shape] = {"tiles"}


@pytest.mark.parametrize("flags", ["address,undefined", "thread"])
def test_tile_table_builders_are_right_and_clean_under_sanitizers(flags, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "schur_tile_tables_driver"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=" + flags, "-fno-omit-frame-pointer", "-I" + CSRC,
           os.path.join(ROOT, "tests", "schur_tile_tables_driver.cpp"), os.path.join(CSRC, "schur_tile_tables.cpp"),
           os.path.join(CSRC, "host_pool.cpp"), "-o", str(exe), "-lpthread"]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if build.returncode != 0 and "sanitizer" in (build.stderr or "").lower() and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("SLAMPP_HIP")}
    args = [str(exe)] + (["threads"] if flags == "thread" else [])
    if flags == "thread" and shutil.which("setarch") is not None:
        # ThreadSanitizer refuses to start ("unexpected memory mapping", before main) where the kernel's address-space
        # randomisation puts a mapping outside the layout it expects: the driver runs without randomisation where it can
        probe = subprocess.run(["setarch", platform.machine(), "-R", "true"], capture_output=True)
        if probe.returncode == 0:
            args = ["setarch", platform.machine(), "-R"] + args
    for _ in range(5):   # (no setarch: started again, a few times at most; nothing of the program has run)
        run = subprocess.run(args, capture_output=True, text=True, timeout=600,
                             env=dict(env, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
        if "FATAL: ThreadSanitizer: unexpected memory mapping" not in run.stderr:
            break
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "WARNING: ThreadSanitizer" not in run.stderr and "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
    lines = run.stdout.splitlines()
    assert all(l.endswith(" ok") for l in lines), run.stdout
    reached = {l.split(":")[0]: set(l.split(" reached", 1)[1].split()[:-1]) for l in lines}
    want_all = THREAD_CASES if flags == "thread" else REACHED
    assert set(reached) == set(want_all), run.stdout
    for name, want in want_all.items():
        assert want <= reached[name], (name, sorted(want - reached[name]))
        assert not (NOT_REACHED.get(name, set()) & reached[name]), (name, sorted(reached[name]))
