"""ctypes binding of vggsfm_amd/csrc/tsdf/vggsfm_amd_tsdf.h (libvggsfm_amd_tsdf.so, built for gfx950): the entries of the
meshing -- TSDF integration of the depth maps and marching tetrahedra on the volume.  A side library
(``_lib.load_side_library``)."""
import ctypes
import os

from ._lib import _D, _I, _INT, _L, _P, check, load_side_library, require_gpu, stream_ptr  # noqa: F401  (re-exported to meshing.py)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvggsfm_amd_tsdf.so")
HEADER = "vggsfm_amd_tsdf.h"
HEADER_PATH = os.path.join(_HERE, "csrc", "tsdf", HEADER)

GROUP, MAX_VIEWS = 256, 256                    # VGGV_GROUP, VGGV_MAX_VIEWS of the header
MAX_NODES = (2 ** 31 - 1) // 7                 # a grid with more nodes is refused

SIGNATURES = {
    "vggv_build_arch": (ctypes.c_char_p, []),
    "vggv_case_table": (_INT, [_P]),
    "vggv_integrate": (_INT, [_P, _P, _P, _P, _P, _I, _I, _I, _D, _D, _D, _D, _I, _I, _I, _D, _P, _P, _P, _P]),
    "vggv_mesh_count": (_INT, [_P, _P, _I, _I, _I, _D, _P, _P, _P, _P, _P, _P, _P]),
    "vggv_mesh_emit": (_INT, [_P, _P, _P, _D, _D, _D, _D, _I, _I, _I, _D, _P, _P, _P, _P, _L, _L, _P, _P, _P, _P, _P]),
}
EXPORTED = list(SIGNATURES)


def lib():
    """Load the meshing's HIP library or fail loudly."""
    return load_side_library(LIB_PATH, SIGNATURES, "vggv_build_arch", "the meshing", "tsdf")
