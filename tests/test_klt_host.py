"""CPU tests of the tracker: what its C-ABI registry has of its own (the registry itself is tests/test_side_libraries.py's),
the yardstick of the GPU tests (the NumPy restatement of tests/klt_cases.py) against analytic truth, and the loud failure of
the product module without the library.  No kernel is called here."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import klt_cases as C
from tests.test_c_abi import _parse_header
from vggsfm_amd import _lib_klt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_table_and_library_agree():
    """What only the tracker has (tests/test_side_libraries.py compares table, header and symbols): two prototypes pinned by
    hand, and the header's constants against the binding and the restatement."""
    header = open(_lib_klt.HEADER_PATH).read()
    functions, _ = _parse_header(header)
    assert functions["vggk_lk_track"][1][7] == "long" and functions["vggk_pyramid_floats"] == ("size_t", ["int"] * 3)
    consts = dict(re.findall(r"#define VGGK_(\w+) (\d+)", header))
    assert [int(consts[k]) for k in ("OK", "FLAT", "LEFT", "DIVERGED", "NONFINITE", "MAX_LEVELS", "MAX_RADIUS")] == \
        [_lib_klt.OK, _lib_klt.FLAT, _lib_klt.LEFT, _lib_klt.DIVERGED, _lib_klt.NONFINITE, _lib_klt.MAX_LEVELS,
         _lib_klt.MAX_RADIUS] == [C.OK, C.FLAT, C.LEFT, C.DIVERGED, C.NONFINITE, 8, 7]


def test_pyramid_sizes_are_computed_on_the_host():
    """vggk_pyramid_floats (host code, no device): the layout of vggsfm_amd.klt.Pyramid and of the restatement; 0 where the
    level count is refused (a level built from a 1 x 1 level, levels outside 1 .. 8)."""
    L = _lib_klt.lib()
    for (h, w), levels, want in (((96, 128), 3, 96 * 128 + 48 * 64 + 24 * 32), ((33, 47), 3, 33 * 47 + 17 * 24 + 9 * 12),
                                 ((1, 9), 5, 9 + 5 + 3 + 2 + 1), ((1, 9), 6, 0), ((2, 2), 2, 5), ((2, 2), 3, 0),
                                 ((5, 7), 4, 35 + 12 + 4 + 1), ((5, 7), 5, 0), ((8, 8), 0, 0), ((8, 8), 9, 0), ((0, 8), 1, 0)):
        assert L.vggk_pyramid_floats(h, w, levels) == want, (h, w, levels)
        if want:
            assert C.flat_pyramid(C.pyramid(np.zeros((1, 1, h, w), np.float32), levels)).shape == (1, want)
        elif h > 0:
            with pytest.raises(ValueError):
                C.pyramid(np.zeros((1, 1, h, w), np.float32), levels)


def test_restatement_against_truth_pure_translation():
    """The yardstick itself: 96 x 128 frames of 70 blobs translated by (7.3, -5.2) px, r = 7, 3 levels, epsilon = 0.01:
    every track within 0.1 px of the analytic motion (measured: max 0.031 px, median 0.009 px)."""
    frames, centres, shift = C.translation_case()
    pyr = C.pyramid(frames, 3)
    pos, status, zncc, iters, _ = C.lk_track([l[0] for l in pyr], [l[1] for l in pyr], centres, radius=7, epsilon=0.01)
    err = np.hypot(*(pos - centres - shift).T)
    print(f"\nmax {err.max():.4f} px, median {np.median(err):.4f} px, iterations <= {iters.max()}")
    assert (status == C.OK).all() and err.max() <= 0.1 and zncc.min() > 0.99


def test_restatement_chain_against_truth():
    """track_features restated, on the 6-frame translation sequence (12 px in all): all visible, within 0.1 px."""
    frames, centres, shifts = C.sequence_case()
    track, vis, score = C.track_features(frames, centres)
    err = np.hypot(*(track - (centres[None] + shifts[:, None])).transpose(2, 0, 1))
    print(f"\nmax {err.max():.4f} px")
    assert vis.all() and err.max() <= 0.1 and score.min() >= 0.9


def test_import_without_the_library_fails_loudly(tmp_path):
    """A copy of the package without libvggsfm_amd_klt.so: importing vggsfm_amd.klt raises the error of _lib.lib(), naming
    the missing file and the build command; there is no fallback."""
    import shutil
    pkg = tmp_path / "vggsfm_amd"
    pkg.mkdir()
    src = os.path.join(ROOT, "vggsfm_amd")
    for name in ("_lib.py", "_lib_klt.py", "klt.py"):
        shutil.copy(os.path.join(src, name), pkg / name)
    (pkg / "__init__.py").write_text("")
    code = ("import sys; sys.path.insert(0, sys.argv[1])\n"
            "try:\n    import vggsfm_amd.klt\nexcept RuntimeError as e:\n    print('RuntimeError:', e)\nelse:\n    print('imported')\n")
    out = subprocess.run([sys.executable, "-c", code, str(tmp_path)], capture_output=True, text=True, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("RuntimeError:") and "libvggsfm_amd_klt.so is missing" in out.stdout \
        and "no CPU or eager fallback" in out.stdout, out.stdout
