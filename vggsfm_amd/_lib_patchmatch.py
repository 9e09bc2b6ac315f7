"""ctypes binding of vggsfm_amd/csrc/patchmatch/vggsfm_amd_patchmatch.h (libvggsfm_amd_pm.so, built for gfx950): the
entries of the PatchMatch slanted-plane refinement of the multi-view stereo.  A side library (``_lib.load_side_library``)."""
import ctypes
import os

from ._lib import _D, _I, _INT, _P, _U, check, load_side_library, require_gpu, stream_ptr  # noqa: F401  (re-exported to patchmatch.py)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvggsfm_amd_pm.so")
HEADER = "vggsfm_amd_patchmatch.h"
HEADER_PATH = os.path.join(_HERE, "csrc", "patchmatch", HEADER)

MAX_SOURCES, MAX_RADIUS = 8, 3                 # VGGR_MAX_* of the header

SIGNATURES = {
    "vggr_build_arch": (ctypes.c_char_p, []),
    "vggr_plane_init": (_INT, [_P, _P, _P, _P, _I, _I, _I, _I, _D, _D, _D, _U, _P, _P]),
    "vggr_plane_cost": (_INT, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _I, _I, _D, _P, _P, _P]),
    "vggr_step": (_INT, [_P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _I, _I, _D, _D, _D, _D, _D, _D, _U, _I, _I, _P, _P, _P]),
    "vggr_outputs": (_INT, [_P, _P, _P, _P, _I, _I, _I, _I, _D, _P, _P, _P, _P]),
}
EXPORTED = list(SIGNATURES)


def lib():
    """Load the PatchMatch refinement's HIP library or fail loudly."""
    return load_side_library(LIB_PATH, SIGNATURES, "vggr_build_arch", "the PatchMatch refinement", "patchmatch")
