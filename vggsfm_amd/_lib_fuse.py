"""ctypes binding of vggsfm_amd/csrc/fuse/vggsfm_amd_fuse.h (libvggsfm_amd_fuse.so, built for gfx950): the entries of the
depth-map fusion.

A library and a table of their own, like the tracker's and the stereo's: the entries of the other libraries and the headers
under include/ are closed, counted sets (tests/test_c_abi.py, tests/test_klt_host.py, tests/test_mvs_host.py).  The
parameter types, ``check``, ``stream_ptr`` and ``require_gpu`` are ``_lib``'s; as there, there is NO fallback: a missing
library or one built for another target raises.  tests/test_fusion_host.py compares the table with the header type by type
and with the library's symbols."""
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
