"""The compiler's resource report of the two-wave leaf backward kernel (csrc/simt_kernel.hip: backward_simt_kernel_branches),
compiled for gfx950 the way the Makefile compiles it: no scratch -- its two register sets fill the file, as the fetch-ahead
form's do, and it is the first to spill when something around it grows -- and one wave a SIMD; and the kernels that were
there before it keep the registers and the occupancy they had: what its helpers' new arguments (the place of a column in its
task) and the shared table staging must not cost them.  No GPU needed; skipped without hipcc."""
import re

from resource_util import report_fixture

UNITS = ("simt_kernel.hip",)

report = report_fixture(UNITS, "simt_bwd_branches_resources")

# kernel<arguments> -> (VGPRs, AGPRs, waves a SIMD) as compiled before the two-wave form joined the unit
BEFORE = {
    "backward_simt_ahead_kernel": {(6, 16, 2): (256, 256, 1), (6, 32, 2): (256, 256, 1), (6, 64, 2): (256, 256, 1)},
    "backward_simt_kernel": {(3, 16): (84, 0, 5), (3, 32): (84, 0, 5), (3, 64): (84, 0, 5), (6, 16): (152, 0, 3), (6, 32): (152, 0, 3),
                             (6, 64): (152, 0, 3), (7, 16): (196, 0, 2), (7, 32): (196, 0, 2), (7, 64): (196, 0, 2)},
    "factor_simt_kernel": {(6, 16, 2, 0): (240, 0, 2), (6, 16, 2, 1): (240, 0, 2), (6, 32, 2, 0): (240, 0, 2), (6, 32, 2, 1): (240, 0, 2)},
}


def instantiations(report, kernel):
    """{template arguments: resources} of a kernel template of namespace slampp with integer and bool arguments."""
    out = {}
    for name, res in report.items():
        m = re.match(rf"_ZN6slampp{len(kernel)}{kernel}I((?:L[ib]\d+E)+)E", name)
        if m:
            out[tuple(int(v) for v in re.findall(r"L[ib](\d+)E", m.group(1)))] = res
    return out


def test_the_two_wave_backward_kernel_has_no_scratch(report):
    mine = instantiations(report, "backward_simt_kernel_branches")
    assert set(mine) == {(6, 16, 2), (6, 32, 2)}, sorted(mine)
    for args, res in sorted(mine.items()):
        print(args, res)
        assert res["ScratchSize"] == 0 and res["Occupancy"] == 1, (args, res)
        assert res["VGPRs"] + res["AGPRs"] <= 512, (args, res)


def test_the_kernels_before_it_keep_their_registers_and_occupancy(report):
    for kernel, want in BEFORE.items():
        got = instantiations(report, kernel)
        assert set(want) <= set(got), (kernel, sorted(got))
        for args, (vgprs, agprs, waves) in want.items():
            res = got[args]
            assert (res["VGPRs"], res["AGPRs"], res["Occupancy"], res["ScratchSize"]) == (vgprs, agprs, waves, 0), (kernel, args, res)
