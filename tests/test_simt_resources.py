"""The compiler's resource report of the lane-per-task kernels (csrc/simt_kernel.hip), compiled for gfx950 the way the Makefile
compiles them: no instantiation of the factor and backward kernels may use scratch -- the fetch-ahead form of the backward
kernel (backward_simt_ahead_kernel) keeps two columns' operands in registers and is the first to spill when it grows --, and
the factor kernel of C3's leaf stage keeps two waves a SIMD; its register allocation has been seen to move when other kernels
joined its translation unit (csrc/dense_tiles.hip says why that happens).  No GPU needed; skipped without hipcc."""
from resource_util import report_fixture

UNITS = ("simt_kernel.hip",)              # every unit that holds a factor_simt or backward_simt kernel

report = report_fixture(UNITS, "simt_resources")


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
