"""The split threshold and chunk length of the device product's long rows are named in three places -- the C header, the
kernel's own header and the Python mirror --: they must say the same."""
import os
import re

from slam_plus_plus_amd import hip_solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_long_row_constants_agree():
    header = open(os.path.join(ROOT, "include", "slampp_hip.h")).read()
    kernel = open(os.path.join(ROOT, "slam_plus_plus_amd", "csrc", "multiply.h")).read()
    for name, value in (("LONG_ROW", hip_solver.MULTIPLY_LONG_ROW), ("CHUNK", hip_solver.MULTIPLY_CHUNK)):
        assert int(re.search(rf"#define SLAMPP_HIP_MULTIPLY_{name} (\d+)", header).group(1)) == value
        assert int(re.search(rf"multiply_{name} = (\d+)", kernel).group(1)) == value
    assert hip_solver.MULTIPLY_CHUNK <= hip_solver.MULTIPLY_LONG_ROW     # a long row has at least two chunks
