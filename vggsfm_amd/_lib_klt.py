"""ctypes binding of vggsfm_amd/csrc/klt/vggsfm_amd_klt.h (libvggsfm_amd_klt.so, built for gfx950): the tracker's entries.
A side library (``_lib.load_side_library``)."""
import ctypes
import os

from ._lib import _D, _I, _INT, _L, _P, _SIZE, _Z, check, load_side_library, require_gpu, stream_ptr  # noqa: F401  (re-exported to klt.py)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvggsfm_amd_klt.so")
HEADER = "vggsfm_amd_klt.h"
HEADER_PATH = os.path.join(_HERE, "csrc", "klt", HEADER)

MAX_LEVELS, MAX_RADIUS = 8, 7                                   # VGGK_MAX_* of the header
OK, FLAT, LEFT, DIVERGED, NONFINITE = range(5)                  # VGGK_* track status

SIGNATURES = {
    "vggk_build_arch": (ctypes.c_char_p, []),
    "vggk_pyramid_floats": (_SIZE, [_I, _I, _I]),
    "vggk_pyramid": (_INT, [_P, _I, _I, _I, _I, _I, _P, _P]),
    "vggk_corner_response": (_INT, [_P, _I, _I, _I, _P, _P]),
    "vggk_local_maxima": (_INT, [_P, _I, _I, _I, _I, _D, _P, _P, _P, _P]),
    "vggk_lk_track": (_INT, [_P, _P, _I, _I, _I, _P, _P, _L, _I, _I, _D, _D, _D, _P, _P, _P, _P, _P]),
}
EXPORTED = list(SIGNATURES)


def lib():
    """Load the tracker's HIP library or fail loudly."""
    return load_side_library(LIB_PATH, SIGNATURES, "vggk_build_arch", "the tracker", "klt")
