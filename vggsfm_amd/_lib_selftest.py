"""ctypes binding of vggsfm_amd/csrc/selftest/vggsfm_amd_selftest.h (libvggsfm_amd_selftest.so, built for gfx950): entries
that run the shared __device__ helpers of csrc/ on a caller's data, for the tests.  A side library
(``_lib.load_side_library``)."""
import ctypes
import os

from ._lib import _I, _INT, _P, check, load_side_library, require_gpu, stream_ptr  # noqa: F401  (re-exported to the tests)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvggsfm_amd_selftest.so")
HEADER = "vggsfm_amd_selftest.h"
HEADER_PATH = os.path.join(_HERE, "csrc", "selftest", HEADER)

# VGGS_* rows of vggs_crosslane's output
GROUP_SUM_8, GROUP_SUM_16, GROUP_SUM_32, GROUP_SUM_64, WAVE_SUM, WAVE_MAX, WAVE_BCAST, NUM_PRIMS = range(8)
SCATTER_VALUES = (6, 14, 24, 28, 36, 45)

SIGNATURES = {
    "vggs_build_arch": (ctypes.c_char_p, []),
    "vggs_crosslane": (_INT, [_P, _P, _I, _I, _P, _I, _P, _P, _P]),
}
EXPORTED = list(SIGNATURES)


def lib():
    """Load the self-test HIP library or fail loudly."""
    return load_side_library(LIB_PATH, SIGNATURES, "vggs_build_arch", "the device self-tests", "selftest")
