"""Writes tests/golden/pnp_epnp.npz for the EPnP tests.  The file is written with fixed zip time stamps: the same script
gives the same bytes.

  python scripts/make_golden_pnp.py

The reference's own ``efficient_pnp`` (vggsfm/two_view_geo/perspective_n_points.py:321-437) is imported through
oracle.ref_harness and run on the CPU in float64.  The two PyTorch3D names its module imports (``oputil.wmean`` and
``points_alignment.corresponding_points_alignment``: PyTorch3D is not installed, the harness can only fabricate it) are
replaced by the stand-ins of tests/pnp_cases.py, a weighted mean and Umeyama with scale; everything else is the
reference's code.  Per case (tests/pnp_cases.py GOLDEN_CASES, B = 7 problems each) the file holds the inputs (x, y, masks,
skip), the true pose, the reference's five outputs (x_cam, R, T, err_2d, err_3d) and the four kernel vectors its
``_null_space`` returned on the way (ref_kernel (B,12,4)): their signs are the eigensolver's and decide whether case 3 gives
a pose, so a comparison with another solver has to know them.
"""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402
from scripts.make_golden_essential import save_npz  # noqa: E402
from tests import pnp_cases as PC  # noqa: E402


def reference_module():
    ref_harness.install()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        import vggsfm.two_view_geo.perspective_n_points as RP
    RP.oputil, RP.points_alignment = PC.pytorch3d_stand_ins()
    return RP


def make():
    """name/key -> array: everything the file holds"""
    RP = reference_module()
    arrays = {}
    for name, c in PC.golden_inputs().items():
        masks = None if c["masks"] is None else torch.from_numpy(c["masks"].astype(np.float64))
        kernels, inner = [], RP._null_space

        def recording(m, kernel_dim):
            kernels.append(inner(m, kernel_dim))
            return kernels[-1]
        RP._null_space = recording
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sol = RP.efficient_pnp(torch.from_numpy(c["x"]), torch.from_numpy(c["y"]), masks=masks,
                                   skip_quadratic_eq=c["skip"])
        RP._null_space = inner
        arrays[f"{name}/ref_kernel"] = kernels[0][0].reshape(-1, 12, 4).numpy()
        for k in ("x", "y", "R_true", "T_true"):
            arrays[f"{name}/{k}"] = c[k]
        if c["masks"] is not None:
            arrays[f"{name}/masks"] = c["masks"]
        arrays[f"{name}/skip"] = np.bool_(c["skip"])
        for k in ("x_cam", "R", "T", "err_2d", "err_3d"):
            arrays[f"{name}/ref_{k}"] = getattr(sol, k).numpy()
    return arrays


def main():
    arrays = make()
    save_npz(PC.GOLDEN, arrays)
    print(f"{PC.GOLDEN}: {os.path.getsize(PC.GOLDEN)} bytes, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
