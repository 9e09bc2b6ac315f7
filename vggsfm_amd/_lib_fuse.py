"""ctypes binding of vggsfm_amd/csrc/fuse/vggsfm_amd_fuse.h (libvggsfm_amd_fuse.so, built for gfx950): the entries of the
depth-map fusion.  A side library (``_lib.load_side_library``)."""
import ctypes
import os

from ._lib import _D, _I, _INT, _L as _LONG, _P, check, load_side_library, require_gpu, stream_ptr  # noqa: F401  (re-exported to fusion.py)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvggsfm_amd_fuse.so")
HEADER = "vggsfm_amd_fuse.h"
HEADER_PATH = os.path.join(_HERE, "csrc", "fuse", HEADER)

MAX_SOURCES = 8               # VGGF_MAX_SOURCES of the header
BLOCK = 256                   # pixels per entry of block_counts

SIGNATURES = {
    "vggf_build_arch": (ctypes.c_char_p, []),
    "vggf_depth_normals": (_INT, [_P, _P, _P, _P, _I, _I, _I, _I, _D, _P, _P]),
    "vggf_fuse_view": (_INT, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _D, _D, _D, _I, _P, _P, _P, _P, _P, _P,
                              _P, _P, _LONG, _P, _P, _P, _P, _P, _P, _P]),
}
EXPORTED = list(SIGNATURES)


def lib():
    """Load the fusion's HIP library or fail loudly."""
    return load_side_library(LIB_PATH, SIGNATURES, "vggf_build_arch", "the depth-map fusion", "fuse")
