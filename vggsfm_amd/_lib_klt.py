"""ctypes binding of vggsfm_amd/csrc/klt/vggsfm_amd_klt.h (libvggsfm_amd_klt.so, built for gfx950): the tracker's entries.

A library and a table of their own: the entries of libvggsfm_amd.so and the headers under include/ are a closed, counted set
(tests/test_c_abi.py).  The parameter types, ``check``, ``stream_ptr`` and ``require_gpu`` are ``_lib``'s; as there, there is
NO fallback: a missing library or one built for another target raises.  tests/test_klt_host.py compares the table with the
header type by type and with the library's symbols."""
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
