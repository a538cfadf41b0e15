"""What the tests of the header binding (include/slam/LinearSolver_HIP.h) share: the include paths and defines
oracle/Makefile.ref builds the drop-in driver with, the skip conditions (the reference's headers, the archives build()
compiles from its block matrix into oracle/_ref, g++), a syntax check of a translation unit, and the build and run of
tests/covariance_header_driver.cpp, which runs the binding on the CPU against the stand-ins of tests/capi_standins.h."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _makefile_vars():
    text = open(os.path.join(ROOT, "oracle", "Makefile.ref")).read()
    out = {}
    for name in ("REF", "OUT", "OPT", "CDEFS", "INC", "CHOLMOD_DEFS"):
        m = re.search(r"^%s\s*[?:]?=\s*(.*)$" % name, text, re.M)
        assert m, name
        out[name] = m.group(1).strip()
    m = re.search(r"^REFLIBS\s*:=\s*((?:.*\\\n)*.*)$", text, re.M)
    assert m, "REFLIBS"
    out["REFLIBS"] = m.group(1).replace("\\\n", " ")
    for name in ("OPT", "CDEFS", "INC", "CHOLMOD_DEFS", "REFLIBS"):
        out[name] = out[name].replace("$(REF)", out["REF"]).replace("$(OUT)", os.path.join(ROOT, out["OUT"]))
    return out


def _compiler_flags(need_archives: bool):
    """The g++ flags and the reference's archives; skips the calling test where something is not present."""
    v = _makefile_vars()
    if not os.path.isdir(os.path.join(v["REF"], "include", "slam")):
        pytest.skip("the reference's headers are not present")
    libs = v["REFLIBS"].split()
    if need_archives and not all(os.path.isfile(a) for a in libs):
        pytest.skip("the reference's archives have not been built")
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    flags = ["-w"] + v["OPT"].split() + v["CDEFS"].split() + v["CHOLMOD_DEFS"].split() + \
        ["-I" + os.path.join(ROOT, "include")] + v["INC"].split()
    return flags, libs


def syntax_check(tmp_path, name: str, text: str) -> None:
    """Compiles the translation unit ``text`` against the reference's headers (g++ -fsyntax-only)."""
    flags, _ = _compiler_flags(False)
    src = tmp_path / name
    src.write_text(text)
    r = subprocess.run(["g++", "-fsyntax-only"] + flags + [str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def run_covariance_driver(tmp_path_factory, *args: str) -> None:
    """Builds tests/covariance_header_driver.cpp (once per test session) and runs it with ``args``: it must print "ok"."""
    flags, libs = _compiler_flags(True)
    exe = tmp_path_factory.getbasetemp() / "covariance_header_driver"
    if not exe.exists():
        partial = tmp_path_factory.mktemp("header_driver") / "covariance_header_driver"
        cmd = ["g++"] + flags + [os.path.join(ROOT, "tests", "covariance_header_driver.cpp"), "-o", str(partial)] + libs + ["-lrt", "-lm"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        os.replace(partial, exe)
    r = subprocess.run([str(exe)] + list(args), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:] + r.stderr[-4000:]
