"""The compiler's resource report of the lane-per-task kernels (csrc/simt_kernel.hip), compiled for gfx950 the way the Makefile
compiles them: no instantiation of the factor and backward kernels may use scratch -- the fetch-ahead form of the backward
kernel (backward_simt_ahead_kernel) keeps two columns' operands in registers and is the first to spill when it grows --, and
the factor kernel of C3's leaf stage keeps two waves a SIMD; its register allocation has been seen to move when other kernels
joined its translation unit (csrc/dense_tiles.hip says why that happens).  No GPU needed; skipped without hipcc."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slam_plus_plus_amd", "csrc")
UNITS = ("simt_kernel.hip",)              # every unit that holds a factor_simt or backward_simt kernel


def makefile_flags():
    """CXXFLAGS of csrc/Makefile with $(ARCH) filled in."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^CXXFLAGS\s*:=\s*(.*)$", text, re.M).group(1).replace("$(ARCH)", arch).split()
    assert f"--offload-arch={arch}" in flags and arch == "gfx950"
    return flags


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out_dir = tmp_path_factory.mktemp("simt_resources")
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


def test_no_lane_per_task_kernel_uses_scratch(report):
    mine = {k: v for k, v in report.items() if "backward_simt" in k or "factor_simt" in k}
    assert any("backward_simt_kernel" in k for k in mine) and any("backward_simt_ahead_kernel" in k for k in mine)
    assert any("factor_simt_kernel" in k for k in mine)
    for k, v in sorted(mine.items()):
        print(k.split("EEEv")[0], v)
    spills = {k: v for k, v in mine.items() if v["ScratchSize"] != 0}
    assert not spills, spills


def test_the_leaf_factor_kernel_keeps_two_waves_a_simd(report):
    hits = [v for k, v in report.items() if "factor_simt_kernelILi6ELi32ELi2ELb0E" in k]     # <6, 32, 2, false>
    assert len(hits) == 1, list(report)
    assert hits[0]["Occupancy"] >= 2 and hits[0]["ScratchSize"] == 0, hits[0]
