"""The compiler's resource report of the fetch-ahead form of the lane-per-task factor kernel (csrc/simt_factor_ahead.hip),
compiled for gfx950 the way the Makefile compiles it: a column's accumulators and the next column's register set share the
register file of one wave a SIMD, and no instantiation of factor_simt_kernel_ahead may use scratch.  The unit is in the
Makefile's source list.  No GPU needed; skipped without hipcc."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam_plus_plus_amd", "csrc")
UNITS = ("simt_factor_ahead.hip",)        # every unit that holds a factor_simt_kernel_ahead instantiation


def makefile_flags():
    """CXXFLAGS of csrc/Makefile with $(ARCH) filled in."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^CXXFLAGS\s*:=\s*(.*)$", text, re.M).group(1).replace("$(ARCH)", arch).split()
    assert f"--offload-arch={arch}" in flags and arch == "gfx950"
    sources = re.search(r"^SRC\s*:=\s*(.*)$", text, re.M).group(1).split()
    assert all(unit in sources for unit in UNITS), sources
    return flags


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out_dir = tmp_path_factory.mktemp("factor_simt_ahead_resources")
    kernels, name = {}, None
    for unit in UNITS:
        out = subprocess.run([hipcc] + makefile_flags() + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage",
                                                           "-o", str(out_dir / "x.o"), os.path.join(CSRC, unit)],
                             capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        for line in out.stderr.splitlines():
            m = re.search(r"remark:\s+Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                kernels[name] = {}
            m = re.search(r"remark:\s+(VGPRs|AGPRs|Occupancy \[waves/SIMD\]|ScratchSize \[bytes/lane\]): (\d+)", line)
            if m and name:
                kernels[name][m.group(1).split(" [")[0]] = int(m.group(2))
    return kernels


def test_no_fetch_ahead_factor_kernel_uses_scratch(report):
    mine = {k: v for k, v in report.items() if "factor_simt_kernel_ahead" in k}
    # block size 6, two lanes per task, the widths a paired launch has, with and without the stored inverses
    for needle in ("ILi6ELi16ELi2ELb0E", "ILi6ELi16ELi2ELb1E", "ILi6ELi32ELi2ELb0E", "ILi6ELi32ELi2ELb1E"):
        assert sum(1 for k in mine if "factor_simt_kernel_ahead" + needle in k) == 1, (needle, sorted(mine))
    for k, v in sorted(mine.items()):
        print(k.split("EEvPK")[0], v)
    for k, v in mine.items():
        assert v["ScratchSize"] == 0 and v["Occupancy"] >= 1 and v["VGPRs"] + v["AGPRs"] <= 512, (k, v)
