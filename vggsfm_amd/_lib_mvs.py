"""ctypes binding of vggsfm_amd/csrc/mvs/vggsfm_amd_mvs.h (libvggsfm_amd_mvs.so, built for gfx950): the entries of the
plane-sweep multi-view stereo.

A library and a table of their own, like the tracker's: the entries of libvggsfm_amd.so and the headers under include/ are a
closed, counted set (tests/test_c_abi.py), and so are the tracker's (tests/test_klt_host.py).  The parameter types, ``check``,
``stream_ptr`` and ``require_gpu`` are ``_lib``'s; as there, there is NO fallback: a missing library or one built for another
target raises.  tests/test_mvs_host.py compares the table with the header type by type and with the library's symbols."""
import ctypes
import os

from ._lib import _D, _I, _INT, _P, check, load_side_library, require_gpu, stream_ptr  # noqa: F401  (re-exported to mvs.py)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvggsfm_amd_mvs.so")
HEADER = "vggsfm_amd_mvs.h"
HEADER_PATH = os.path.join(_HERE, "csrc", "mvs", HEADER)

MAX_SOURCES, MAX_PLANES, MAX_RADIUS = 8, 1024, 3               # VGGM_MAX_* of the header

SIGNATURES = {
    "vggm_build_arch": (ctypes.c_char_p, []),
    "vggm_plane_sweep": (_INT, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _D, _D, _I, _I, _I, _D, _D, _P, _P, _P, _P, _P]),
    "vggm_consistency_filter": (_INT, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _D, _D, _I, _P, _P, _P]),
}
EXPORTED = list(SIGNATURES)


def lib():
    """Load the multi-view stereo HIP library or fail loudly."""
    return load_side_library(LIB_PATH, SIGNATURES, "vggm_build_arch", "the multi-view stereo", "mvs")
