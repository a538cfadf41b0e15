"""The compiler's resource report of the fetch-ahead form of the lane-per-task factor kernel (csrc/simt_factor_ahead.hip),
compiled for gfx950 the way the Makefile compiles it: a column's accumulators and the next column's register set share the
register file of one wave a SIMD, and no instantiation of factor_simt_kernel_ahead may use scratch.  The unit is in the
Makefile's source list.  No GPU needed; skipped without hipcc."""
from resource_util import report_fixture

UNITS = ("simt_factor_ahead.hip",)        # every unit that holds a factor_simt_kernel_ahead instantiation

report = report_fixture(UNITS, "factor_simt_ahead_resources")


def test_no_fetch_ahead_factor_kernel_uses_scratch(report):
    mine = {k: v for k, v in report.items() if "factor_simt_kernel_ahead" in k}
    # block size 6, two lanes per task, the widths a paired launch has, with and without the stored inverses
    for needle in ("ILi6ELi16ELi2ELb0E", "ILi6ELi16ELi2ELb1E", "ILi6ELi32ELi2ELb0E", "ILi6ELi32ELi2ELb1E"):
        assert sum(1 for k in mine if "factor_simt_kernel_ahead" + needle in k) == 1, (needle, sorted(mine))
    for k, v in sorted(mine.items()):
        print(k.split("EEvPK")[0], v)
    for k, v in mine.items():
        assert v["ScratchSize"] == 0 and v["Occupancy"] >= 1 and v["VGPRs"] + v["AGPRs"] <= 512, (k, v)
