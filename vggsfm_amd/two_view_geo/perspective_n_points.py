"""EPnP on the device (vggsfm/two_view_geo/perspective_n_points.py: ``efficient_pnp``), host side of ``vggp_epnp_solve``
(csrc/epnp.hip).  All problems of a call run concurrently, one workgroup each.

Differences from the reference: the computation is float64 whatever the input dtype and the
result is cast to the input dtype; ``masks`` selects points (non-zero = used), and what a masked-out slot holds never
reaches the result (its slot of ``x_cam`` is 0); a problem that cannot be solved (fewer than 4 used points, or a
candidate that is not finite) returns the identity, zeros and infinite errors, as ``run_5point`` returns the identity.
"""
from typing import NamedTuple, Optional

import torch

from .. import _lib


class EpnpSolution(NamedTuple):
    x_cam: torch.Tensor
    R: torch.Tensor
    T: torch.Tensor
    err_2d: torch.Tensor
    err_3d: torch.Tensor


def epnp_solve(x, y, masks=None, skip_quadratic_eq=False, return_x_cam=True):
    """``vggp_epnp_solve``: x (B,N,3) or (N,3) shared by all problems, y (B,N,2), masks (B,N) or None.  Everything float64.
    Returns (EpnpSolution, variant (B,) int32, valid (B,) bool); x_cam is None when not asked for."""
    if y.dim() != 3 or y.shape[-1] != 2:
        raise ValueError(f"y must be (B,N,2), got {tuple(y.shape)}")
    B, N, _ = y.shape
    shared = x.dim() == 2
    if tuple(x.shape) != ((N, 3) if shared else (B, N, 3)):
        raise ValueError(f"x must be (B,N,3) or (N,3) with y (B,N,2), got {tuple(x.shape)} and {tuple(y.shape)}")
    if N < 4:
        raise ValueError(f"need at least 4 points, got {N}")
    if masks is not None and tuple(masks.shape) != (B, N):
        raise ValueError("masks must be (B,N)")
    _lib.require_gpu(x, y, masks)
    L = _lib.lib()
    dev = y.device
    xd, yd = x.to(torch.float64).contiguous(), y.to(torch.float64).contiguous()
    w = None if masks is None else (masks != 0).to(torch.uint8).contiguous()
    R = torch.empty((B, 3, 3), dtype=torch.float64, device=dev)
    T = torch.empty((B, 3), dtype=torch.float64, device=dev)
    e2 = torch.empty(B, dtype=torch.float64, device=dev)
    e3 = torch.empty(B, dtype=torch.float64, device=dev)
    xc = torch.empty((B, N, 3), dtype=torch.float64, device=dev) if return_x_cam else None
    variant = torch.empty(B, dtype=torch.int32, device=dev)
    valid = torch.empty(B, dtype=torch.uint8, device=dev)
    _lib.check(L.vggp_epnp_solve(xd, int(shared), yd, w, B, N, int(bool(skip_quadratic_eq)), R, T, e2, e3, xc, variant, valid,
                                 _lib.stream_ptr()), "vggp_epnp_solve")
    return EpnpSolution(xc, R, T, e2, e3), variant, valid.bool()


def efficient_pnp(
    x: torch.Tensor,
    y: torch.Tensor,
    masks: Optional[torch.Tensor] = None,
    weights: Optional[torch.Tensor] = None,
    skip_quadratic_eq: bool = False,
) -> EpnpSolution:
    """perspective_n_points.py:321-437: R (B,3,3), T (B,3) with ``y = Proj(x R + T)``, x_cam (B,N,3), err_2d, err_3d (B,),
    in the dtype of ``x``.  ``weights`` is ignored, as in the reference, which overwrites it with ``masks``."""
    sol, _, _ = epnp_solve(x, y, masks, skip_quadratic_eq)
    return EpnpSolution(*(t.to(x.dtype) for t in sol))
