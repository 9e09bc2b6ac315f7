"""ctypes binding of vggsfm_amd/csrc/icp/vggsfm_amd_icp.h (libvggsfm_amd_icp.so, built for gfx950): the entries of the
registration library -- the fused ICP step against a point grid or a triangle grid (transform, grid walk, residual, Jacobian
row and the normal equations in one kernel), the sums of its workspace, the Gauss-Newton update of the device-resident
transform, and the radius normals of a point grid.  A side library (``_lib.load_side_library``)."""
import ctypes
import os

from ._lib import _D, _I, _INT, _P, check, load_side_library, require_gpu, stream_ptr  # noqa: F401  (re-exported to registration.py)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvggsfm_amd_icp.so")
HEADER = "vggsfm_amd_icp.h"
HEADER_PATH = os.path.join(_HERE, "csrc", "icp", HEADER)

# VGGI_GROUPS, VGGI_BLOCK, VGGI_WORDS, VGGI_STATE_WORDS, VGGI_HISTORY_WORDS, VGGI_NORMAL_SWEEPS of the header
GROUPS, BLOCK, WORDS, STATE_WORDS, HISTORY_WORDS, NORMAL_SWEEPS = 512, 256, 40, 18, 7, 8
PIVOT_MIN = 1e-12
STATUS = ("running", "converged", "too few", "degenerate")      # VGGI_RUNNING .. VGGI_DEGENERATE

_GRID = [_D, _D, _D, _D, _I, _I, _I]           # ox, oy, oz, cell, d0, d1, d2
_STEP = [_P, _D, _D, _I, _I, _I, _D, _P, _P, _P]   # state, max_dist, r2, metric, estimate_scale, loss, loss_scale, ws, out, stream

SIGNATURES = {
    "vggi_build_arch": (ctypes.c_char_p, []),
    "vggi_icp_step": (_INT, [_P, _P, _I, _P, _P, _P, _I] + _GRID + [_P] + _STEP),
    "vggi_icp_step_mesh": (_INT, [_P, _P, _I, _P, _I, _P, _I, _P, _P, _I] + _GRID + _STEP),
    "vggi_icp_sums": (_INT, [_P, _P, _P]),
    "vggi_icp_update": (_INT, [_P, _P, _I, _I, _D, _D, _D, _D, _P, _I, _P]),
    "vggi_radius_normals": (_INT, [_P, _P, _P, _I] + _GRID + [_D, _D, _I, _P, _P, _P, _P, _P]),
}
EXPORTED = list(SIGNATURES)


def lib():
    """Load the registration HIP library or fail loudly."""
    return load_side_library(LIB_PATH, SIGNATURES, "vggi_build_arch", "the dense registration (ICP)", "icp")
