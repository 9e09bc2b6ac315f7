"""CPU test of the device self-tests' C-ABI registry: vggsfm_amd/_lib_selftest.py against csrc/selftest/vggsfm_amd_selftest.h
and the dynamic symbols of libvggsfm_amd_selftest.so.  No kernel is called here."""
import os
import re
import subprocess

from tests.test_c_abi import _parse_header, _table_kinds
from vggsfm_amd import _lib, _lib_selftest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_table_and_library_agree():
    header = open(_lib_selftest.HEADER_PATH).read()
    functions, structs = _parse_header(header)
    table = _table_kinds(_lib_selftest.SIGNATURES)
    assert list(table) == list(functions) and len(functions) == 2 and not structs
    for name in functions:
        assert table[name] == functions[name], name
        assert name.startswith("vggs_"), name
    assert os.path.exists(_lib_selftest.LIB_PATH), "run __graft_entry__.build() first"
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib_selftest.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert set(re.findall(r" T (vgg[a-z]?_\w+)$", nm, flags=re.M)) == set(_lib_selftest.SIGNATURES)
    assert not set(_lib_selftest.SIGNATURES) & set(_lib.SIGNATURES)
    assert _lib_selftest.HEADER not in os.listdir(os.path.join(ROOT, "include"))
    L = _lib_selftest.lib()
    assert L.vggs_build_arch() == b"gfx950"
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
