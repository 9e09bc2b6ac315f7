"""CPU tests of the device self-tests: the rows of vggs_crosslane's output in csrc/selftest/vggsfm_amd_selftest.h against
vggsfm_amd/_lib_selftest.py (the registry itself is tests/test_side_libraries.py's), and where the bundle adjustment takes its
cross-lane sums from.  No kernel is called here."""
import os
import re

from vggsfm_amd import _lib_selftest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_table_and_library_agree():
    header = open(_lib_selftest.HEADER_PATH).read()
    consts = dict(re.findall(r"#define VGGS_(\w+) (\d+)", header))
    names = ("GROUP_SUM_8", "GROUP_SUM_16", "GROUP_SUM_32", "GROUP_SUM_64", "WAVE_SUM", "WAVE_MAX", "WAVE_BCAST", "NUM_PRIMS")
    assert [int(consts[k]) for k in names] == [getattr(_lib_selftest, k) for k in names] == list(range(8))


def test_the_ba_units_take_their_cross_lane_sums_from_the_one_header():
    """No __shfl on doubles is left in the bundle adjustment's sources or in the shared headers they include."""
    csrc = os.path.join(ROOT, "vggsfm_amd", "csrc")
    for name in ("ba.hip", "ba_cam.hip", "ba_point.hip", "ba_tiles.hip", "ba_exchange.hip", "ba_obs.hpp", "ba_types.hpp",
                 "crosslane.hpp"):
        text = open(os.path.join(csrc, name)).read()
        code = re.sub(r"//[^\n]*", "", text)
        assert "__shfl" not in code, name
    common = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "common.hpp")).read())
    assert re.findall(r"__shfl\w*\(", common) == ["__shfl_xor("] and "wave_sum_i" in common     # (the 32-bit integer sum)
