"""What the compiler-resource tests share (test_simt_resources.py, test_factor_simt_ahead_resources.py): the Makefile's flags and
the compiler's resource report of some units of csrc/, compiled for gfx950 the way the Makefile compiles them.  A plain module,
imported by those tests; no GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam_plus_plus_amd", "csrc")


def makefile_flags(units=()):
    """CXXFLAGS of csrc/Makefile with $(ARCH) filled in; units: sources that must be in the Makefile's list."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^CXXFLAGS\s*:=\s*(.*)$", text, re.M).group(1).replace("$(ARCH)", arch).split()
    assert f"--offload-arch={arch}" in flags and arch == "gfx950"
    sources = re.search(r"^SRC\s*:=\s*(.*)$", text, re.M).group(1).split()
    assert all(unit in sources for unit in units), sources
    return flags


def report_fixture(units, name):
    """A module-scoped fixture: {kernel: {VGPRs, AGPRs, Occupancy, ScratchSize}} of the units; skips without hipcc."""
    @pytest.fixture(scope="module")
    def report(tmp_path_factory):
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            pytest.skip("no hipcc")
        out_dir = tmp_path_factory.mktemp(name)
        kernels, kernel = {}, None
        for unit in units:
            out = subprocess.run([hipcc] + makefile_flags(units) + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                                                                    "-o", str(out_dir / "x.o"), os.path.join(CSRC, unit)],
                                 capture_output=True, text=True, timeout=900)
            assert out.returncode == 0, out.stderr[-2000:]
            for line in out.stderr.splitlines():
                m = re.search(r"remark:\s+Function Name: (\S+)", line)
                if m:
                    kernel = m.group(1)
                    kernels[kernel] = {}
                m = re.search(r"remark:\s+(VGPRs|AGPRs|Occupancy \[waves/SIMD\]|ScratchSize \[bytes/lane\]): (\d+)", line)
                if m and kernel:
                    kernels[kernel][m.group(1).split(" [")[0]] = int(m.group(2))
        return kernels
    return report
