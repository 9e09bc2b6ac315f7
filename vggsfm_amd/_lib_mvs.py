"""ctypes binding of vggsfm_amd/csrc/mvs/vggsfm_amd_mvs.h (libvggsfm_amd_mvs.so, built for gfx950): the entries of the
plane-sweep multi-view stereo.  A side library (``_lib.load_side_library``)."""
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
