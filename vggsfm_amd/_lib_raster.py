"""ctypes binding of vggsfm_amd/csrc/raster/vggsfm_amd_raster.h (libvggsfm_amd_raster.so, built for gfx950): the entries of
the rasteriser -- a mesh drawn into the views of a reconstruction through a z-buffer of 64-bit keys, the buffer resolved to
depth, face, normal and colour maps, and the visibility of points against depth maps.  A side library
(``_lib.load_side_library``)."""
import ctypes
import os

from ._lib import _D, _I, _INT, _P, check, load_side_library, require_gpu, stream_ptr  # noqa: F401  (re-exported to render.py)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvggsfm_amd_raster.so")
HEADER = "vggsfm_amd_raster.h"
HEADER_PATH = os.path.join(_HERE, "csrc", "raster", HEADER)

MAX_VIEWS, SOLO_PIXELS = 256, 64               # VGGZ_MAX_VIEWS, VGGZ_SOLO_PIXELS of the header
MAX_FACES = 2 ** 31 - 1                        # face_base + num_faces beyond this is refused

SIGNATURES = {
    "vggz_build_arch": (ctypes.c_char_p, []),
    "vggz_raster": (_INT, [_P, _I, _P, _I, _I, _P, _P, _P, _P, _I, _I, _I, _I, _D, _P, _P]),
    "vggz_resolve": (_INT, [_P, _P, _I, _P, _I, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "vggz_point_visibility": (_INT, [_P, _I, _P, _P, _P, _I, _I, _I, _D, _P, _P]),
}
EXPORTED = list(SIGNATURES)


def lib():
    """Load the rasteriser's HIP library or fail loudly."""
    return load_side_library(LIB_PATH, SIGNATURES, "vggz_build_arch", "the rasteriser", "raster")
