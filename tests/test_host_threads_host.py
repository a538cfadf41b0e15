"""The fork-join helper of the host passes (csrc/host_threads.h) on the CPU, under sanitizers.  The header is plain C++, so
tests/host_threads_driver.cpp -- a program of its own -- is compiled here with g++ -fsanitize=address,undefined and, second
case, =thread, and run: the ranges of for_ranges, a job that throws std::bad_alloc, the worker count.  Built once more with
-DSLAMPP_HOST_THREADS_TEST_FAIL_AFTER=k (0, and 3 of 8), the header's thread start throws std::system_error(EAGAIN) from the
k-th thread on: every job must still run exactly once, the rest of them on the calling thread."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("fail_after", [None, 0, 3])
@pytest.mark.parametrize("flags", ["address,undefined", "thread"])
def test_host_threads_under_sanitizers(flags, fail_after, tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "host_threads_driver"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=" + flags, "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "slam_plus_plus_amd", "csrc"), os.path.join(ROOT, "tests", "host_threads_driver.cpp"),
           "-o", str(exe), "-lpthread"]
    if fail_after is not None:
        cmd.insert(1, "-DSLAMPP_HOST_THREADS_TEST_FAIL_AFTER=%d" % fail_after)
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "sanitizer" in (build.stderr or "").lower() and "cannot find" in build.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert build.returncode == 0, build.stderr[-2000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("SLAMPP_HIP_DEV")}
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600,
                         env=dict(env, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "WARNING: ThreadSanitizer" not in run.stderr and "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
    assert "host_threads_driver: ok" in run.stdout
