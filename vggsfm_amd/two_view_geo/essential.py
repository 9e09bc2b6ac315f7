"""``estimate_essential`` on the device (vggsfm/two_view_geo/essential.py:111-488): 5-point RANSAC, one round of local
optimisation (the same 5-point solve on X^T X summed over a hypothesis' inliers), winner by (inlier count, mean inlier
residual) -- every image pair of the batch at once.  Host side of ``vgge_emat_five_point`` / ``vgge_emat_score`` /
``vgge_emat_refine`` / ``vgge_emat_solve`` (csrc/essential.hip) and of ``vgg_fmat_residuals`` for the winner; the only
host-side step between the launches is the stable sort that selects the lo_num best hypotheses.

Two deliberate deviations from the reference: only the REAL roots of the degree-10 polynomial
give candidates (the reference also builds candidates from the real parts of complex roots), and scoring is float64 (the
reference scores in float32)."""
import torch

from .. import _lib
from .utils import generate_samples, pick_winner, select_best


def _score(L, p1, p2, E, valid, thr):
    B, N = p1.shape[0], p1.shape[1]
    K = E.shape[1]
    cnt = torch.empty((B, K), dtype=torch.int32, device=p1.device)
    rs = torch.empty((B, K), dtype=torch.float64, device=p1.device)
    _lib.check(L.vgge_emat_score(p1, p2, E, valid, thr, B, N, K, cnt, rs, _lib.stream_ptr()), "vgge_emat_score")
    return cnt, rs


def _five_point(L, p1, p2, smp):
    """p1, p2 (B,N,2) float64 normalised, smp (H,5) int32 -> candidates (B,10H,9), flags (B,10H)."""
    B, N = p1.shape[0], p1.shape[1]
    H = int(smp.shape[0])
    E = torch.empty((B, H, 10, 9), dtype=torch.float64, device=p1.device)
    ok = torch.empty((B, H, 10), dtype=torch.uint8, device=p1.device)
    _lib.check(L.vgge_emat_five_point(p1, p2, smp, B, N, H, E, ok, _lib.stream_ptr()), "vgge_emat_five_point")
    return E.reshape(B, 10 * H, 9), ok.reshape(B, 10 * H)


def _refine(L, p1, p2, Esrc, cnt_src, order, thr):
    """The 5-point solve on the inliers of hypotheses order (B,lo) int32 of Esrc -> candidates (B,10 lo,9), flags."""
    B, N = p1.shape[0], p1.shape[1]
    K, lo = Esrc.shape[1], int(order.shape[1])
    E = torch.empty((B, lo, 10, 9), dtype=torch.float64, device=p1.device)
    ok = torch.empty((B, lo, 10), dtype=torch.uint8, device=p1.device)
    _lib.check(L.vgge_emat_refine(p1, p2, Esrc, cnt_src, order, thr, B, N, K, lo, E, ok, _lib.stream_ptr()),
               "vgge_emat_refine")
    return E.reshape(B, 10 * lo, 9), ok.reshape(B, 10 * lo)


def _normalise(points1, points2, focal_length, principal_point):
    pp, fl = principal_point.to(torch.float64).unsqueeze(1), focal_length.to(torch.float64).unsqueeze(1)
    p1 = ((points1.to(torch.float64) - pp[..., :2]) / fl[..., :2]).contiguous()
    p2 = ((points2.to(torch.float64) - pp[..., 2:]) / fl[..., 2:]).contiguous()
    return p1, p2


def estimate_essential(points1, points2, focal_length, principal_point, max_ransac_iters=1024, max_error=4, lo_num=50, *,
                       samples=None, return_residuals=False):
    """points1, points2 (B,N,2) pixels; focal_length, principal_point (B,4), [:2] the left frame and [2:] the right one.
    Returns (best_emat (B,3,3) of unit Frobenius norm with p2^T E p1 = 0 in normalised coordinates, best_inlier_num (B,),
    best_inlier_mask (B,N) [, residuals (B,N)]), all float64 arithmetic.  The threshold on the squared Sampson distance is
    per pair: (max_error / mean of the pair's four focal lengths)^2.  `samples` (H,5) int overrides the host draw."""
    if points1.dim() != 3 or points1.shape[-1] != 2 or points1.shape != points2.shape:
        raise ValueError(f"points1 and points2 must both be (B,N,2), got {tuple(points1.shape)} and {tuple(points2.shape)}")
    B, N, _ = points1.shape
    if N < 5:
        raise ValueError(f"need at least 5 matches, got {N}")
    if tuple(focal_length.shape) != (B, 4) or tuple(principal_point.shape) != (B, 4):
        raise ValueError("focal_length and principal_point must be (B,4)")
    if int(lo_num) < 0:
        raise ValueError(f"lo_num must be >= 0, got {lo_num}")
    if samples is not None and (getattr(samples, "ndim", 0) != 2 or samples.shape[1] != 5 or samples.shape[0] < 1):
        raise ValueError("samples must be (H,5) with H >= 1")
    _lib.require_gpu(points1, points2, focal_length, principal_point)
    L = _lib.lib()
    dev = points1.device
    p1, p2 = _normalise(points1, points2, focal_length, principal_point)
    thr = ((float(max_error) / focal_length.to(torch.float64).mean(dim=-1)) ** 2).contiguous()
    if samples is None:
        samples = generate_samples(N, max_ransac_iters, 5)
    smp = torch.as_tensor(samples, dtype=torch.int32, device=dev).contiguous()
    Ea, va = _five_point(L, p1, p2, smp)
    cnt, rs = _score(L, p1, p2, Ea, va, thr)
    lo = min(int(lo_num), Ea.shape[1])
    Eall, call, rall = Ea, cnt, rs
    if lo > 0:                                  # (lo_num = 0: no local optimisation, as in the reference)
        El, vl = _refine(L, p1, p2, Ea, cnt, select_best(cnt, lo), thr)
        cl, rl = _score(L, p1, p2, El, vl, thr)
        Eall, call, rall = torch.cat([Ea, El], 1), torch.cat([cnt, cl], 1), torch.cat([rs, rl], 1)
    Eb, num, mask, res = pick_winner(p1, p2, None, Eall, call, rall, thr)
    if return_residuals:
        return Eb.reshape(B, 3, 3), num, mask, res
    return Eb.reshape(B, 3, 3), num, mask


def run_5point(points1, points2, masks=None, weights=None, *, return_valid=False):
    """essential.py:203-264: normalised points (B,N,2), N >= 5; `masks` (B,N) multiplies the rows of the linear system.
    Returns (B,10,3,3): the candidates of the real roots first, the identity in the unused slots (as the reference fills
    a set it could not solve); with return_valid also the (B,10) bool flags."""
    if weights is not None:
        raise NotImplementedError("run_5point: weights are not implemented (the reference never passes them)")
    if points1.dim() != 3 or points1.shape[-1] != 2 or points1.shape != points2.shape:
        raise ValueError(f"points1 and points2 must both be (B,N,2), got {tuple(points1.shape)} and {tuple(points2.shape)}")
    B, N, _ = points1.shape
    if N < 5:
        raise ValueError(f"need at least 5 points, got {N}")
    if masks is not None and tuple(masks.shape) != (B, N):
        raise ValueError("masks must be (B,N)")
    _lib.require_gpu(points1, points2, masks)
    L = _lib.lib()
    dev = points1.device
    p1, p2 = points1.to(torch.float64).contiguous(), points2.to(torch.float64).contiguous()
    w = None if masks is None else masks.to(torch.float64).contiguous()
    E = torch.empty((B, 10, 9), dtype=torch.float64, device=dev)
    ok = torch.empty((B, 10), dtype=torch.uint8, device=dev)
    _lib.check(L.vgge_emat_solve(p1, p2, w, B, N, E, ok, _lib.stream_ptr()), "vgge_emat_solve")
    ok = ok.bool()
    eye = torch.eye(3, dtype=torch.float64, device=dev).reshape(1, 1, 9)
    E = torch.where(ok[..., None], E, eye).reshape(B, 10, 3, 3)
    return (E, ok) if return_valid else E


def relative_pose_from_essential(emat, points1, points2, focal_length, principal_point):
    """The (R (B,3,3), t (B,3)) of emat (B,3,3): its four SVD candidates (``decompose_essential_matrix``) and the one with
    the most matches in front of both cameras (``remove_cheirality``).  points in pixels, intrinsics (B,4)."""
    from .estimate_preliminary import decompose_essential_matrix, remove_cheirality
    _lib.require_gpu(emat, points1, points2, focal_length, principal_point)
    Rs, Ts = decompose_essential_matrix(emat)
    return remove_cheirality(Rs, Ts, points1, points2, focal_length, principal_point)
