"""ctypes binding of vggsfm_amd/csrc/nn/vggsfm_amd_nn.h (libvggsfm_amd_nn.so, built for gfx950): the entries of the
nearest-neighbour library -- the cells of points on a uniform grid, the grid's cell_start, the nearest point and the nearest
triangle of the grid for many queries, and the counts and sums over such distances that the dense metrics are made of.  A
side library (``_lib.load_side_library``)."""
import ctypes
import os

from ._lib import _D, _I, _INT, _L, _P, check, load_side_library, require_gpu, stream_ptr  # noqa: F401  (re-exported to nearest.py)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvggsfm_amd_nn.so")
HEADER = "vggsfm_amd_nn.h"
HEADER_PATH = os.path.join(_HERE, "csrc", "nn", HEADER)

# VGGN_MAX_CELLS, VGGN_MAX_THRESHOLDS, VGGN_STATS_GROUPS, VGGN_STATS_WORDS of the header
MAX_CELLS, MAX_THRESHOLDS, STATS_GROUPS, STATS_WORDS = 2 ** 25, 8, 256, 12
MAX_PAIRS = 2 ** 31 - 1                        # (cell, face) pairs of a triangle grid

_GRID = [_D, _D, _D, _D, _I, _I, _I]           # ox, oy, oz, cell, d0, d1, d2

SIGNATURES = {
    "vggn_build_arch": (ctypes.c_char_p, []),
    "vggn_point_cells": (_INT, [_P, _I] + _GRID + [_P, _P]),
    "vggn_gather_points": (_INT, [_P, _P, _I, _P, _P]),
    "vggn_cell_start": (_INT, [_P, _I, _I, _P, _P]),
    "vggn_nearest_point": (_INT, [_P, _P, _P, _I] + _GRID + [_P, _P, _I, _D, _D, _I, _P, _P, _P, _P]),
    "vggn_face_cell_counts": (_INT, [_P, _I, _P, _I] + _GRID + [_P, _P]),
    "vggn_face_cell_pairs": (_INT, [_P, _I, _P, _I] + _GRID + [_P, _L, _P, _P, _P]),
    "vggn_nearest_face": (_INT, [_P, _I, _P, _I, _P, _P, _I] + _GRID + [_P, _P, _I, _D, _D, _P, _P, _P, _P]),
    "vggn_distance_stats": (_INT, [_P, _I, _P, _I, _P, _P, _P, _P]),
}
EXPORTED = list(SIGNATURES)


def lib():
    """Load the nearest-neighbour HIP library or fail loudly."""
    return load_side_library(LIB_PATH, SIGNATURES, "vggn_build_arch", "the nearest-neighbour search", "nn")
